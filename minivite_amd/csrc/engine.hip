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
//
// The K4 kernels and their launch dispatch are sweep.hip's, the multi-phase
// driver is multiphase.hip's (the map of the files: engine_internal.h).

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "cub_util.h"
#include "engine_internal.h"

namespace {

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

// ---- K10a: append the values outside [base, bound) to out: remote tails
// (exchangeVertexReqs, dspl.hpp:1140-1164) and the candidate remote
// communities of an iteration (dspl.hpp:670-700) ----
__global__ void k_select_remote(i64 n, const i64 *__restrict__ vals,
                                i64 base, i64 bound, i64 *__restrict__ out,
                                unsigned long long *__restrict__ count) {
    for (i64 k = blockIdx.x * (i64)blockDim.x + threadIdx.x; k < n;
         k += (i64)gridDim.x * blockDim.x) {
        const i64 v = vals[k];
        if (v < base || v >= bound) out[atomicAdd(count, 1ull)] = v;
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

} // namespace

i64 remote_ids(hipStream_t st, i64 n, const i64 *d_vals, i64 base, i64 bound,
               int bits, DevBuf<i64> &d_ids) {
    DevBuf<i64> d_rem(n), d_sorted; // temporaries: freed at return
    DevBuf<unsigned long long> d_count(1);
    DevBuf<char> d_tmp;
    HIP_CHECK(hipMemsetAsync(d_count, 0, 8, st));
    k_select_remote<<<grid_for(n), 256, 0, st>>>(n, d_vals, base, bound, d_rem,
                                                 d_count);
    const i64 nrem = (i64)read_back(d_count.get(), st);
    d_sorted.reserve(nrem);
    d_ids.reserve(nrem);
    cub_sort_keys(d_tmp, st, d_rem.get(), d_sorted.get(), nrem, bits);
    i64 *d_n = (i64 *)d_count.get(); // reuse as output slot
    cub_unique(d_tmp, st, d_sorted.get(), d_ids.get(), d_n, nrem);
    return read_back(d_n, st);
}

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
    // an explicit window is honoured even where waves then idle
    const i64 S = ws ? std::min<i64>(W / 64, 8)
                     : default_row_group(e->lnv, e->sweep_grid, W);
    if (S < 1) return;
    e->deg_window = W;
    e->deg_quant = q;
    e->row_group = (int)S;
}

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
    } else {
        U = default_sweep_unit(e->lnv, e->sweep_grid);
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
    e->sort_bits = ceil_log2(e->nv);
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
        k_iota<<<grid_for(lnv), 256>>>(lnv, e->d_sigma.get());
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

} // extern "C"

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
void exchange(mv_engine *e, const std::vector<Xfer> &sends,
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
void alltoallv(mv_engine *e, const void *send, const i64 *soff, void *recv,
               const i64 *roff, size_t elem_bytes, ncclDataType_t ty,
               ncclComm_t comm, hipStream_t stream) {
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
void allgather_counts(mv_engine *e, const i64 *mine, bool on_device,
                      i64 *matrix, ncclComm_t comm, hipStream_t stream) {
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
void comm_allreduce_host(mv_engine *e, double *vals, int n) {
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

// ---- build_sell, step by step. Every step works on e->stream; d_tmp is
// the hipCUB temporary they share. ----

// 1. Degree order. perm = identity with a spatial hint (sigma carries the
// order), degree-descending otherwise (load balance for skewed degree
// distributions); then d_sdeg holds the sorted degrees, else it stays null.
// Reads lnv, d_sigma, d_xadj, has_hint, skewed; sets d_deg, d_perm, d_iota,
// perm_identity.
static void sell_degree_order(mv_engine *e, DevBuf<char> &d_tmp,
                              DevBuf<unsigned> &d_sdeg) {
    hipStream_t st = e->stream;
    const i64 lnv = e->lnv;
    k_degrees<<<grid_for(lnv), 256, 0, st>>>(lnv, e->d_sigma, e->d_xadj,
                                             e->d_deg);
    e->perm_identity = e->has_hint && !e->skewed; // until step 3 permutes it
    if (e->perm_identity) {
        k_iota<<<grid_for(lnv), 256, 0, st>>>(lnv, e->d_perm.get());
        return;
    }
    k_iota<<<grid_for(lnv), 256, 0, st>>>(lnv, e->d_iota.get());
    d_sdeg.reserve(lnv);
    cub_sort_pairs_descending(d_tmp, st, e->d_deg.get(), d_sdeg.get(),
                              e->d_iota.get(), e->d_perm.get(), lnv, 32);
}

// 2. High-degree split + per-vertex hash regions of a degree-sorted order
// (unit: wave-per-vertex atomic hash; -w: per-lane serial hash in edge
// order). Reads lnv, lne, skewed, unit_weights, d_tails, base, bound,
// d_sigma_inv, d_ghosts, nghost; sets nhi, nlh, and for nlh > 0 d_tidx32,
// d_hash_off, hash_hub_elems, hash_total, d_hkeys, d_hacc, d_lh_list.
static void sell_hash_bands(mv_engine *e, const DevBuf<unsigned> &d_sdeg) {
    hipStream_t st = e->stream;
    const i64 lnv = e->lnv;
    e->nhi = 0;
    e->nlh = 0;
    if (!d_sdeg) return; // identity order: never skewed
    std::vector<unsigned> sdeg(lnv);
    if (lnv) // a rank may own no vertices (null data())
        HIP_CHECK(hipMemcpyAsync(sdeg.data(), d_sdeg, 4 * lnv,
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
    if (e->nlh == 0) return;
    e->d_tidx32.reserve(e->lne);
    k_translate_tails<<<grid_for(e->lne), 256, 0, st>>>(
        e->lne, e->d_tails, e->base, e->bound, e->d_sigma_inv, e->d_ghosts,
        e->nghost, lnv, e->d_tidx32);
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
    HIP_CHECK(hipMemcpyAsync(e->d_hash_off, hoff.data(), 8 * (e->nlh + 1),
                             hipMemcpyHostToDevice, st));
    e->hash_total = acc;
    if (e->d_hkeys.reserve(acc)) { // the three grow together
        e->d_hacc.reserve(acc);
        e->d_lh_list.reserve(acc / 2 + 1);
    }
    HIP_CHECK(hipStreamSynchronize(st));
}

// 3. Exports-first SELL order (halo overlap): positions [0, nexp) hold
// the vertices some peer wants (the svdata set), so the sweep can run
// them as a first launch and halo #1a for the NEXT iteration — which
// only needs their targets — can overlap the interior sweep + the
// whole epilogue on stream2/comm2 (north_star: "#1a overlapped with
// the local sweep on a second HIP stream"). Stable partition: locality
// inside each group is preserved. Pure layout, results identical.
// Reads lnv, nranks, skewed, ssz, d_svdata_int, comm2 / lb; sets nexp,
// overlap, and when it partitions d_perm, perm_identity.
static void sell_exports_first(mv_engine *e, DevBuf<char> &d_tmp) {
    hipStream_t st = e->stream;
    const i64 lnv = e->lnv;
    e->nexp = 0;
    e->overlap = 0;
    if (e->nranks == 1 || e->skewed || e->ssz == 0 || !has_second_channel(e) ||
        getenv("MV_NO_OVERLAP"))
        return;
    // device-side stable partition (two hipCUB Flagged selects): the
    // host round trip cost ~ms per run at 8-GPU sizes
    DevBuf<unsigned char> d_mark(lnv), d_flags(lnv); // freed at return
    DevBuf<unsigned> d_out(lnv);
    DevBuf<i64> d_num(1);
    HIP_CHECK(hipMemsetAsync(d_mark, 0, lnv, st));
    k_scatter_mark<<<grid_for(e->ssz), 256, 0, st>>>(e->ssz, e->d_svdata_int,
                                                     d_mark);
    k_gather_flags<<<grid_for(lnv), 256, 0, st>>>(lnv, e->d_perm, d_mark,
                                                  d_flags, 0);
    cub_select_flagged(d_tmp, st, e->d_perm.get(), d_flags.get(), d_out.get(),
                       d_num.get(), lnv);
    e->nexp = read_back(d_num.get(), st);
    k_gather_flags<<<grid_for(lnv), 256, 0, st>>>(lnv, e->d_perm, d_mark,
                                                  d_flags, 1);
    cub_select_flagged(d_tmp, st, e->d_perm.get(), d_flags.get(),
                       d_out + e->nexp, d_num.get(), lnv);
    HIP_CHECK(hipMemcpyAsync(e->d_perm, d_out, 4 * lnv,
                             hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    e->overlap = 1;
    e->perm_identity = 0;
}

// 4. The SELL image over d_perm: slice offsets, tails translated inline,
// and for unit graphs the row sort. Reads lnv, nchunks, d_perm, d_deg,
// d_sigma, d_sigma_inv, d_xadj, d_tails, d_ew, base, bound, d_ghosts,
// nghost, unit_weights, skewed; sets d_chunk_off, sell_entries,
// d_sell_tidx, d_sell_w, sell_sorted.
static void sell_fill_image(mv_engine *e, DevBuf<char> &d_tmp) {
    hipStream_t st = e->stream;
    const i64 lnv = e->lnv;
    DevBuf<i64> d_sizes(e->nchunks); // freed at return
    k_chunk_sizes<<<grid_for(e->nchunks), 256, 0, st>>>(
        e->nchunks, lnv, e->d_perm, e->d_deg, d_sizes);
    HIP_CHECK(hipMemsetAsync(e->d_chunk_off, 0, 8, st));
    cub_inclusive_sum(d_tmp, st, d_sizes.get(), e->d_chunk_off + 1,
                      e->nchunks);
    const i64 total = read_back(e->d_chunk_off + e->nchunks, st);
    e->sell_entries = total;
    e->d_sell_tidx.reserve(total);
    if (!e->unit_weights) e->d_sell_w.reserve(total);
    k_fill_sell<<<grid_for(lnv), 256, 0, st>>>(
        lnv, e->d_perm, e->d_sigma, e->d_sigma_inv, e->d_xadj, e->d_tails,
        e->d_ew, e->base, e->bound, e->d_ghosts, e->nghost, e->d_chunk_off,
        e->d_sell_tidx, e->unit_weights ? nullptr : e->d_sell_w.get());
    // unit graphs: re-sort rows by internal index for gather locality
    // (see k_sell_sort_rows; results identical, measured +4-5%)
    e->sell_sorted = 0;
    if (e->unit_weights && !e->skewed && !getenv("MV_NO_ROWSORT")) {
        k_sell_sort_rows<<<grid_for(lnv), 256, 0, st>>>(
            lnv, e->d_perm, e->d_deg, e->d_chunk_off, e->d_sell_tidx);
        e->sell_sorted = 1;
    }
}

// 5. Per-thread spill extents of K4. Reads lnv, sweep_grid, skewed,
// max_degree, nlh, d_perm, d_deg; sets d_spill_off, d_spill_k, d_spill_a.
static void sell_spill_extents(mv_engine *e) {
    hipStream_t st = e->stream;
    const i64 nthreads = (i64)e->sweep_grid * 256;
    i64 total;
    if (!e->skewed) {
        const i64 per = std::max<i64>(e->max_degree, 1);
        k_spill_uniform<<<grid_for(nthreads), 256, 0, st>>>(nthreads, per,
                                                            e->d_spill_off);
        total = nthreads * per;
    } else {
        DevBuf<i64> d_need(nthreads); // freed with this block
        k_spill_need<<<grid_for(nthreads), 256, 0, st>>>(
            nthreads, e->nlh, e->lnv, e->d_perm, e->d_deg, 4, d_need);
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
        HIP_CHECK(hipMemcpyAsync(e->d_spill_off, off.data(), 8 * nthreads,
                                 hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    e->d_spill_k.reserve(total);
    e->d_spill_a.reserve(total);
}

// Build the SELL image, internal order, spill extents and the high-degree
// hash regions. Pure graph-layout preparation (a function of the static
// graph + the ghost list), analogous to the reference's CSR existing
// before its timed span; called at load for single-rank graphs and right
// after ghost discovery inside the span for multi-rank ones (the ghost
// slots feed the tail translation).
static void build_sell(mv_engine *e) {
    DevBuf<char> d_tmp;      // temporaries: freed at return, after the
    DevBuf<unsigned> d_sdeg; // stream has drained
    sell_degree_order(e, d_tmp, d_sdeg);
    sell_hash_bands(e, d_sdeg);
    sell_exports_first(e, d_tmp);
    sell_fill_image(e, d_tmp);
    sell_spill_extents(e);
    HIP_CHECK(hipStreamSynchronize(e->stream));
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
        // the sort + unique below never have more than cand_max ids: sized
        // here, d_cub_tmp does not grow (a hipFree would device-sync and
        // re-serialize the overlapped pipeline) before the next load
        cub_presize_sort_unique(e->d_cub_tmp, cand_max, e->sort_bits);
    }
    // two sources, ghost labels then curr, into one candidate array
    HIP_CHECK(hipMemsetAsync(e->d_count, 0, 8, st2));
    k_select_remote<<<grid_for(std::max<i64>(e->nghost, 1)), 256, 0, st2>>>(
        e->nghost, e->d_ghost_labels, e->base, e->bound, e->d_cand,
        e->d_count);
    k_select_remote<<<grid_for(lnv), 256, 0, st2>>>(
        lnv, curr, e->base, e->bound, e->d_cand, e->d_count);
    const i64 ncand = (i64)read_back(e->d_count.get(), st2);
    cub_sort_keys(e->d_cub_tmp, st2, e->d_cand.get(), e->d_cand_sorted.get(),
                  ncand, e->sort_bits);
    i64 *d_nrc = (i64 *)e->d_count.get(); // reuse as output slot
    cub_unique(e->d_cub_tmp, st2, e->d_cand_sorted.get(), e->d_rc_ids.get(),
               d_nrc, ncand);
    const i64 nrc = read_back(d_nrc, st2);

    // ---- halo #1b/#1c/#1d: request (size,degree) of those communities
    // from their owners (dspl.hpp:719-929) ----
    lower_bounds_device(st2, e->d_rc_ids.get(), nrc, e->d_parts.get(), p + 1,
                        e->d_bounds.get());
    rc_bounds.assign(p + 1, 0);
    HIP_CHECK(hipMemcpyAsync(rc_bounds.data(), e->d_bounds, 8 * (p + 1),
                             hipMemcpyDeviceToHost, st2));
    HIP_CHECK(hipStreamSynchronize(st2));
    std::vector<i64> reqs(p), matrix((size_t)p * p);
    for (int r = 0; r < p; r++) reqs[r] = rc_bounds[r + 1] - rc_bounds[r];
    allgather_counts(e, reqs.data(), /*on_device*/ false, matrix.data(), comm,
                     st2);
    recv_offsets(matrix, p, me, /*with_own*/ false, req_off);
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
    if (p == 1) {
        e->nghost = 0;
        e->ssz = 0;
        return; // the SELL image was built at load
    }
    // ghosts: the sorted distinct remote tails
    e->nghost = remote_ids(st, lne, e->d_tails, e->base, e->bound,
                           e->sort_bits, e->d_ghosts);

    // per-owner segments of my (sorted) want list
    lower_bounds_device(st, e->d_ghosts.get(), e->nghost, e->d_parts.get(),
                        p + 1, e->d_bounds.get());
    e->recv_off.resize(p + 1);
    HIP_CHECK(hipMemcpyAsync(e->recv_off.data(), e->d_bounds, 8 * (p + 1),
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));

    // exchange want-list sizes, then the lists (dspl.hpp:1184-1252)
    std::vector<i64> want(p), matrix((size_t)p * p);
    for (int r = 0; r < p; r++) want[r] = e->recv_off[r + 1] - e->recv_off[r];
    allgather_counts(e, want.data(), /*on_device*/ false, matrix.data(),
                     e->comm, st);
    recv_offsets(matrix, p, me, /*with_own*/ false, e->send_off);
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

// persist the sweep's u32 view targets as labels (p>1 only)
static void writeback(mv_engine *e, i64 s0, i64 s1, i64 *d_target) {
    if (e->nranks == 1 || s1 <= s0) return;
    k_view_to_labels<<<grid_for(s1 - s0, 256, 2048), 256, 0, e->stream>>>(
        s0, s1, e->d_perm, e->d_vtarget, e->d_sigma, e->base, e->d_rc_ids,
        e->lnv, d_target);
}

// an internal-ordered community array as labels in original local order
static void depermute_labels(mv_engine *e, const i64 *src, i64 *dst) {
    const i64 lnv = e->lnv;
    if (e->nranks == 1) // slot mode: u32 slots
        k_depermute32<<<grid_for(lnv), 256, 0, e->stream>>>(
            lnv, e->d_sigma, e->d_sigma_inv, (const unsigned *)src, dst);
    else
        k_depermute<<<grid_for(lnv), 256, 0, e->stream>>>(
            lnv, e->d_sigma_inv, src, dst);
}

// the parity trace of iteration `iter` (mv_engine_set_trace)
static void record_trace(mv_engine *e, int iter, double mod,
                         const i64 *d_target) {
    if (e->trace_mod && iter <= e->trace_cap) e->trace_mod[iter - 1] = mod;
    if (!e->trace_target || iter > e->trace_cap) return;
    depermute_labels(e, d_target, e->d_trace_tmp);
    if (e->lnv)
        HIP_CHECK(hipMemcpyAsync(e->trace_target + (i64)(iter - 1) * e->lnv,
                                 e->d_trace_tmp, 8 * e->lnv,
                                 hipMemcpyDeviceToHost, e->stream));
    HIP_CHECK(hipStreamSynchronize(e->stream));
}

extern "C" double mv_engine_run(mv_engine *e, double lower, double thresh,
                                int *iters_out) {
    HIP_CHECK(hipSetDevice(e->device));
    const auto t_start = clk::now();
    hipStream_t st = e->stream;
    const i64 lnv = e->lnv, lne = e->lne;
    const int p = e->nranks;
    e->ev_used = 0;
    e->stats = mv_stats{};
    e->sweep = mv_sweep_info{};
    e->halo = mv_halo_info{};
    e->stats.edges_local = lne;

    const auto t_setup0 = clk::now();
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
    double totalW = 0.0; // the local sum, block order
    for (int b = 0; b < nblocks; b++) totalW += partials[2 * b];
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
    e->stats.setup_ms = ms_since(t_setup0);
    const SweepPlan plan = sweep_plan(e, constant);
    const bool mod_debug = getenv("MV_MOD_DEBUG") != nullptr;

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

    for (;;) {
        numIters++;

        // ---- halo #1 (dspl.hpp:583-929): wait for it, or exchange ----
        if (p > 1) {
            const auto t_h0 = clk::now();
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
            e->stats.halo_ms += ms_since(t_h0);
        }

        // ---- K4 sweep (dspl.hpp:1371-1387; K5's zeroing is fused: cupd is
        // zeroed by K6 after each apply + once before the loop, and the
        // sweep overwrites clusterWeight instead of accumulating) ----
        if (numIters == 1 && lnv)
            HIP_CHECK(hipMemsetAsync(e->d_cupd, 0, sizeof(Cinfo) * lnv, st));
        hipEvent_t ev0 = e->ev_pair(), ev1 = e->ev_pair();
        HIP_CHECK(hipEventRecord(ev0, st));
        sweep_hash_bands(e, plan, numIters, d_curr, d_target);
        if (p > 1 && e->overlap) {
            // exports first (their targets feed the next iteration's #1a
            // once ev_p1 fires); the full next-iteration pipeline is
            // issued after the epilogue's delta application (ev_cinfo) so
            // it runs under the epilogue + exit check — see below
            sweep_positions(e, plan, numIters, d_curr, d_target, 0, e->nexp);
            writeback(e, 0, e->nexp, d_target);
            HIP_CHECK(hipEventRecord(e->ev_p1, st));
            sweep_positions(e, plan, numIters, d_curr, d_target, e->nexp, lnv);
            writeback(e, e->nexp, lnv, d_target);
            HIP_CHECK(hipEventRecord(e->ev_p2, st));
        } else {
            sweep_positions(e, plan, numIters, d_curr, d_target, e->nlh, lnv);
            writeback(e, 0, lnv, d_target);
        }
        HIP_CHECK(hipEventRecord(ev1, st));
        PHASE("sweep-done");
        e->stats.sweep_launches++;

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
            const auto t_h0 = clk::now();
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
            e->stats.halo_ms += ms_since(t_h0);
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
        double red[2] = {0.0, 0.0}; // le, la: block order, then rank order
        for (int b = 0; b < nblocks; b++) {
            red[0] += partials[2 * b];
            red[1] += partials[2 * b + 1];
        }
        if (p > 1) comm_allreduce_host(e, red, 2);
        currMod = std::fabs(red[0] * constant - red[1] * constant * constant);
        if (mod_debug)
            std::fprintf(stderr, "[mod] iter=%d le=%.17g la=%.17g\n",
                         numIters, red[0], red[1]);
        record_trace(e, numIters, currMod, d_target);

        // ---- exit check, rotate ----
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

    const bool dbg = getenv("MV_SWEEP_DEBUG") != nullptr; // ev_pool: per sweep
    for (int k = 0; k + 1 < e->ev_used; k += 2) {
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, e->ev_pool[k], e->ev_pool[k + 1]));
        e->stats.sweep_ms += ms;
        if (dbg)
            std::fprintf(stderr, "[sweep] iter %d: %.3f ms\n", k / 2 + 1, ms);
    }
    e->res_src = numIters <= 2 ? d_curr : d_past;
    e->stats.iters = numIters;
    e->stats.total_ms = ms_since(t_start);
    *iters_out = numIters;
    return prevMod; // dspl.hpp:1440
}

const i64 *phase_labels_device(mv_engine *e) {
    if (!e->res_src) return nullptr;
    e->d_res.reserve(e->lnv);
    depermute_labels(e, e->res_src, e->d_res);
    return e->d_res;
}
