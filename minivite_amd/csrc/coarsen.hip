// coarsen.hip — community aggregation (graph coarsening) on the MI355X: the
// hot step between two Louvain phases. The reference mini-app stops after
// phase one and has no counterpart; the definitions are DESIGN.md's
// multi-phase section.
//
// Pipeline (sort-based, insensitive to degree skew):
//   1. renumber   scatter-mark used labels, exclusive scan, gather
//                 -> map[v] = dense coarse id in ascending label order
//   2. keys       one 64-bit key (map[u] << b) | map[tail] per directed
//                 edge, b = ceil(log2 nc); edge-parallel, the row of an
//                 edge found per wave (wave-wide row window from xadj,
//                 then a per-lane search inside the window)
//   3. sort       hipCUB radix sort over the 2b live key bits; stable, so
//                 equal keys keep fine-edge order. Unit-weight inputs sort
//                 keys only
//   4. runs       run heads -> exclusive scan -> one coarse edge per run;
//                 row offsets by binary search on the run keys' high half;
//                 weights summed in a FIXED order: a run of <= 32 edges
//                 left to right by one thread, a longer run by one block
//                 (256 strided sequential partials, then a fixed LDS
//                 tree) — no floating-point atomics anywhere, so results
//                 are bit-identical run to run. Unit inputs take the run
//                 length as the weight.
// Temporary storage is O(lne).
//
// Steps 3 and 4 are one building block (mv_sort_reduce_keys) over a
// caller-supplied key/weight array. The distributed aggregation (the
// orchestration and every exchange live in multiphase.hip, over
// engine.hip's transport seam) runs it twice — once over the local edges, once at the
// owner over the received per-rank partials — around the transport-free
// pieces at the end of this file: sort-unique of global ids with the
// scatter back through the sort permutation, owner-bucket bounds, the
// owner-side gather / mark / dense-id kernels, and the key kernel with the
// local / remote tail split.
//
// Device memory, the binary search, the iota and bounds kernels are
// device_util.h's and every hipCUB call goes through cub_util.h: the same
// ones the engine uses. Nothing here needs RCCL or the engine's structs.

#include <vector>

#include "../../include/minivite_hip.h"
#include "coarsen.h"
#include "cub_util.h"

namespace {

using u64 = unsigned long long;

constexpr int kShortRun = 32; // longest run one thread sums on its own

// ---- 1. renumber ----
// used[l] = 1 for every label in use; a label outside [0,nv) raises *err
// and is not written
__global__ void k_mark_labels(i64 nv, const i64 *__restrict__ labels,
                              unsigned *__restrict__ used,
                              unsigned *__restrict__ err) {
    for (i64 v = blockIdx.x * (i64)blockDim.x + threadIdx.x; v < nv;
         v += (i64)gridDim.x * blockDim.x) {
        const i64 l = labels[v];
        if (l < 0 || l >= nv) *err = 1u;
        else used[l] = 1u;
    }
}

__global__ void k_gather_map(i64 nv, const i64 *__restrict__ labels,
                             const unsigned *__restrict__ rank,
                             i64 *__restrict__ map) {
    for (i64 v = blockIdx.x * (i64)blockDim.x + threadIdx.x; v < nv;
         v += (i64)gridDim.x * blockDim.x)
        map[v] = (i64)rank[labels[v]];
}

// ---- 2. key generation ----
// largest r in [lo, hi] with xadj[r] <= e (xadj[lo] <= e is given); empty
// rows (equal offsets) are skipped because the LAST such r is taken
__device__ __forceinline__ i64 row_of(const i64 *__restrict__ xadj, i64 lo,
                                      i64 hi, i64 e) {
    while (lo < hi) {
        const i64 mid = (lo + hi + 1) >> 1;
        if (xadj[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// One wave owns a tile of 64 consecutive edges: the rows of the tile's
// first and last edge bound a window (wave-uniform searches over the whole
// xadj), and each lane then places its own edge inside that window — a hub
// row costs its waves one window of width 1, never a serial walk.
__global__ __launch_bounds__(256) void k_coarse_keys(
    i64 nv, i64 lne, const i64 *__restrict__ xadj,
    const i64 *__restrict__ tails, const i64 *__restrict__ map, int shift,
    u64 *__restrict__ keys) {
    const int lane = threadIdx.x & 63;
    const i64 wave = (blockIdx.x * (i64)blockDim.x + threadIdx.x) >> 6;
    const i64 nwaves = ((i64)gridDim.x * blockDim.x) >> 6;
    for (i64 e0 = wave * 64; e0 < lne; e0 += nwaves * 64) {
        const i64 e1 = e0 + 63 < lne ? e0 + 63 : lne - 1;
        const i64 r0 = row_of(xadj, 0, nv - 1, e0);
        const i64 r1 = row_of(xadj, r0, nv - 1, e1);
        const i64 e = e0 + lane;
        if (e <= e1) {
            const i64 r = row_of(xadj, r0, r1, e);
            keys[e] = ((u64)map[r] << shift) | (u64)map[tails[e]];
        }
    }
}

// ---- 4. runs ----
// head[i] = 1 where a run of equal keys starts; head[lne] = 0 closes the
// scan so that its last output is the run count
__global__ void k_run_heads(i64 lne, const u64 *__restrict__ ks,
                            unsigned *__restrict__ head) {
    for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i <= lne;
         i += (i64)gridDim.x * blockDim.x)
        head[i] = (i < lne && (i == 0 || ks[i] != ks[i - 1])) ? 1u : 0u;
}

// run j = pos[i] of head i: its first sorted edge and its key;
// run_start[nruns] = lne closes the last run
__global__ void k_run_fill(i64 lne, const u64 *__restrict__ ks,
                           const unsigned *__restrict__ head,
                           const unsigned *__restrict__ pos,
                           i64 *__restrict__ run_start,
                           u64 *__restrict__ run_key) {
    for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i <= lne;
         i += (i64)gridDim.x * blockDim.x) {
        if (i == lne) {
            run_start[pos[lne]] = lne;
        } else if (head[i]) {
            run_start[pos[i]] = i;
            run_key[pos[i]] = ks[i];
        }
    }
}

// coarse row offsets (first run whose high key half is >= row0 + c, c in
// [0, nc]) and tails (the low key half of each run); row0 = 0 and nc = all
// rows on a single rank, the owned range of a partitioned level
__global__ void k_coarse_rows(i64 row0, i64 nc, i64 nruns, int shift,
                              const u64 *__restrict__ run_key,
                              i64 *__restrict__ cxadj,
                              i64 *__restrict__ ctails) {
    const u64 mask = (1ull << shift) - 1ull;
    const i64 n = nruns > nc + 1 ? nruns : nc + 1;
    for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < n;
         i += (i64)gridDim.x * blockDim.x) {
        if (i <= nc)
            cxadj[i] = dev_lower_bound(run_key, nruns,
                                       (u64)(row0 + i) << shift);
        if (i < nruns) ctails[i] = (i64)(run_key[i] & mask);
    }
}

// unit inputs: the weight of a coarse edge is the number of fine edges
__global__ void k_run_lengths(i64 nruns, const i64 *__restrict__ run_start,
                              double *__restrict__ cw) {
    for (i64 j = blockIdx.x * (i64)blockDim.x + threadIdx.x; j < nruns;
         j += (i64)gridDim.x * blockDim.x)
        cw[j] = (double)(run_start[j + 1] - run_start[j]);
}

// short runs: one thread, left to right; longer runs are queued (the queue
// order is arbitrary, each queued run's sum is not)
__global__ void k_reduce_short(i64 nruns, const i64 *__restrict__ run_start,
                               const double *__restrict__ ws,
                               double *__restrict__ cw,
                               i64 *__restrict__ long_list,
                               u64 *__restrict__ long_count) {
    for (i64 j = blockIdx.x * (i64)blockDim.x + threadIdx.x; j < nruns;
         j += (i64)gridDim.x * blockDim.x) {
        const i64 s = run_start[j], t = run_start[j + 1];
        if (t - s > kShortRun) {
            long_list[atomicAdd(long_count, 1ull)] = j;
            continue;
        }
        double a = 0.0;
        for (i64 i = s; i < t; i++) a += ws[i];
        cw[j] = a;
    }
}

// long runs: one block per run at a time, any length — thread t sums
// elements s+t, s+t+256, ... in order, then a fixed 256-leaf LDS tree
__global__ __launch_bounds__(256) void k_reduce_long(
    const i64 *__restrict__ long_list, const u64 *__restrict__ long_count,
    const i64 *__restrict__ run_start, const double *__restrict__ ws,
    double *__restrict__ cw) {
    __shared__ double sb[256];
    const i64 n = (i64)*long_count;
    for (i64 k = blockIdx.x; k < n; k += gridDim.x) {
        const i64 j = long_list[k];
        const i64 s = run_start[j], t = run_start[j + 1];
        double a = 0.0;
        for (i64 i = s + threadIdx.x; i < t; i += 256) a += ws[i];
        sb[threadIdx.x] = a;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off)
                sb[threadIdx.x] += sb[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x == 0) cw[j] = sb[0];
        __syncthreads();
    }
}

} // namespace

void mv_sort_reduce_keys(hipStream_t st, int64_t n, const uint64_t *d_keys_in,
                         const double *d_w, int bits, mv_key_runs *out) {
    *out = mv_key_runs{};
    if (n == 0) { // never-null outputs
        out->d_key.reserve(0);
        out->d_w.reserve(0);
        return;
    }
    const u64 *keys = (const u64 *)d_keys_in;
    // ---- 3. sort over the live key bits ----
    DevBuf<u64> ks(n);
    DevBuf<double> ws(d_w ? n : 0);
    DevBuf<char> tmp; // freed at return: every path below synchronises
    if (d_w)
        cub_sort_pairs(tmp, st, keys, ks.get(), d_w, ws.get(), n, bits);
    else
        cub_sort_keys(tmp, st, keys, ks.get(), n, bits);

    // ---- 4. runs ----
    DevBuf<unsigned> head(n + 1), pos(n + 1);
    k_run_heads<<<grid_for(n + 1), 256, 0, st>>>(n, ks, head);
    mv_exclusive_sum_u32(st, head, pos, n + 1);
    const i64 nruns = read_back(pos + n, st);
    out->n = nruns;
    out->d_key.reserve(nruns);
    out->d_w.reserve(nruns);
    DevBuf<i64> run_start(nruns + 1);
    k_run_fill<<<grid_for(n + 1), 256, 0, st>>>(n, ks, head, pos, run_start,
                                                (u64 *)out->d_key.get());
    if (!d_w) {
        k_run_lengths<<<grid_for(nruns), 256, 0, st>>>(nruns, run_start,
                                                       out->d_w);
        HIP_CHECK(hipStreamSynchronize(st));
    } else {
        DevBuf<i64> long_list(nruns);
        DevBuf<u64> long_count(1);
        HIP_CHECK(hipMemsetAsync(long_count, 0, 8, st));
        k_reduce_short<<<grid_for(nruns), 256, 0, st>>>(
            nruns, run_start, ws, out->d_w, long_list, long_count);
        k_reduce_long<<<grid_for(nruns, 1, 1024), 256, 0, st>>>(
            long_list, long_count, run_start, ws, out->d_w);
        HIP_CHECK(hipStreamSynchronize(st));
    }
}

int mv_coarsen_device(hipStream_t st, int64_t nv, int64_t lne,
                      const int64_t *d_xadj, const int64_t *d_tails,
                      const double *d_w, const int64_t *d_labels,
                      bool stop_if_identity, mv_coarse_dev *out) {
    *out = mv_coarse_dev{};
    if (nv < 1 || nv >= (1ll << 31) || lne < 0 || lne >= (1ll << 31) - 1) {
        std::fprintf(stderr,
                     "mv_coarsen: need 1 <= nv < 2^31 and lne < 2^31 - 1 "
                     "(nv=%lld lne=%lld)\n",
                     (long long)nv, (long long)lne);
        return -1;
    }

    // ---- 1. renumber ----
    DevBuf<unsigned> used(nv + 2), rank(nv + 1);
    unsigned *err = used + nv + 1; // one word past the scan's closing 0
    HIP_CHECK(hipMemsetAsync(used, 0, 4 * (nv + 2), st));
    k_mark_labels<<<grid_for(nv), 256, 0, st>>>(nv, d_labels, used, err);
    mv_exclusive_sum_u32(st, used, rank, nv + 1);
    const i64 nc = read_back(rank + nv, st);
    if (read_back(err, st)) {
        std::fprintf(stderr,
                     "mv_coarsen: community label outside [0, nv=%lld)\n",
                     (long long)nv);
        return -1;
    }
    out->nc = nc;
    out->d_map.reserve(nv);
    k_gather_map<<<grid_for(nv), 256, 0, st>>>(nv, d_labels, rank,
                                               out->d_map);
    if (stop_if_identity && nc == nv) {
        HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    }

    // ---- 2./3. keys + sort over the 2*shift live bits ----
    const int shift = ceil_log2(nc);
    out->d_xadj.reserve(nc + 1);
    if (lne == 0) {
        HIP_CHECK(hipMemsetAsync(out->d_xadj, 0, 8 * (nc + 1), st));
        HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    }
    DevBuf<u64> keys(lne);
    k_coarse_keys<<<grid_for(lne), 256, 0, st>>>(nv, lne, d_xadj, d_tails,
                                                 out->d_map, shift, keys);
    mv_key_runs runs;
    mv_sort_reduce_keys(st, lne, (const uint64_t *)keys.get(), d_w, 2 * shift,
                        &runs);
    const i64 nruns = runs.n;
    out->ne = nruns;
    out->d_tails.reserve(nruns);
    k_coarse_rows<<<grid_for(std::max(nruns, nc + 1)), 256, 0, st>>>(
        0, nc, nruns, shift, (const u64 *)runs.d_key.get(), out->d_xadj,
        out->d_tails);
    HIP_CHECK(hipStreamSynchronize(st));
    out->d_w = std::move(runs.d_w); // the run weights ARE the coarse weights
    return 0;
}

extern "C" mv_graph *mv_coarsen_csr(int device, const mv_graph *g,
                                    const int64_t *comm, int64_t *map_out) {
    const i64 nv = mv_graph_nv(g), lne = mv_graph_lne(g);
    if (mv_graph_lnv(g) != nv) {
        std::fprintf(stderr, "mv_coarsen_csr: single-rank graphs only "
                             "(lnv != nv)\n");
        return nullptr;
    }
    const i64 *xadj = mv_graph_xadj(g), *tails = mv_graph_tails(g);
    const double *w = mv_graph_weights(g);
    for (i64 k = 0; k < lne; k++)
        if (tails[k] < 0 || tails[k] >= nv) {
            std::fprintf(stderr, "mv_coarsen_csr: tail out of range\n");
            return nullptr;
        }
    if (xadj[0] != 0 || xadj[nv] != lne) {
        std::fprintf(stderr, "mv_coarsen_csr: malformed xadj\n");
        return nullptr;
    }
    for (i64 v = 0; v < nv; v++)
        if (xadj[v] > xadj[v + 1]) {
            std::fprintf(stderr, "mv_coarsen_csr: malformed xadj\n");
            return nullptr;
        }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) {
        std::fprintf(stderr,
                     "mv_coarsen_csr: no HIP device %d (found %d). There is "
                     "no CPU fallback.\n",
                     device, ndev);
        return nullptr;
    }
    HIP_CHECK(hipSetDevice(device));
    bool unit = true;
    for (i64 k = 0; k < lne && unit; k++) unit = w[k] == 1.0;

    hipStream_t st = nullptr; // the default stream: a one-shot entry
    DevBuf<i64> d_xadj(nv + 1), d_tails(lne), d_comm(nv);
    DevBuf<double> d_w(unit ? 0 : lne);
    HIP_CHECK(hipMemcpy(d_xadj, xadj, 8 * (nv + 1), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_tails, tails, 8 * lne, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_comm, comm, 8 * nv, hipMemcpyHostToDevice));
    if (!unit) HIP_CHECK(hipMemcpy(d_w, w, 8 * lne, hipMemcpyHostToDevice));

    mv_coarse_dev c;
    if (mv_coarsen_device(st, nv, lne, d_xadj, d_tails,
                          unit ? nullptr : d_w.get(), d_comm, false, &c) != 0)
        return nullptr;
    std::vector<i64> cx(c.nc + 1), ct(c.ne);
    std::vector<double> cw(c.ne);
    HIP_CHECK(hipMemcpy(map_out, c.d_map, 8 * nv, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(cx.data(), c.d_xadj, 8 * (c.nc + 1),
                        hipMemcpyDeviceToHost));
    if (c.ne) {
        HIP_CHECK(hipMemcpy(ct.data(), c.d_tails, 8 * c.ne,
                            hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(cw.data(), c.d_w, 8 * c.ne,
                            hipMemcpyDeviceToHost));
    }
    const i64 parts[2] = {0, c.nc};
    return mv_graph_from_csr(c.nc, 0, 1, parts, c.nc, c.ne, cx.data(),
                             ct.data(), cw.data());
}

// ------------------------------------------------------------------------
// Transport-free pieces of the distributed aggregation (multiphase.hip
// strings them together across the seam; DESIGN.md, multi-phase section).

namespace {

// heads of the runs of equal sorted ids; head[n] = 0 closes the scan
__global__ void k_id_heads(i64 n, const i64 *__restrict__ s,
                           unsigned *__restrict__ head) {
    for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i <= n;
         i += (i64)gridDim.x * blockDim.x)
        head[i] = (i < n && (i == 0 || s[i] != s[i - 1])) ? 1u : 0u;
}

// run[i] = index of sorted entry i's run; uniq[run] = the id at its head
__global__ void k_id_runs(i64 n, const i64 *__restrict__ s,
                          const unsigned *__restrict__ head,
                          const unsigned *__restrict__ pos,
                          unsigned *__restrict__ run,
                          i64 *__restrict__ uniq) {
    for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < n;
         i += (i64)gridDim.x * blockDim.x) {
        const unsigned r = pos[i] + head[i] - 1u;
        run[i] = r;
        if (head[i]) uniq[r] = s[i];
    }
}

__global__ void k_scatter_unique(i64 n, const unsigned *__restrict__ perm,
                                 const unsigned *__restrict__ run,
                                 const i64 *__restrict__ vals,
                                 i64 *__restrict__ out) {
    for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < n;
         i += (i64)gridDim.x * blockDim.x)
        out[perm[i]] = vals[run[i]];
}

__global__ void k_gather_owned(i64 n, const i64 *__restrict__ ids, i64 base,
                               const i64 *__restrict__ table,
                               i64 *__restrict__ out) {
    for (i64 k = blockIdx.x * (i64)blockDim.x + threadIdx.x; k < n;
         k += (i64)gridDim.x * blockDim.x)
        out[k] = table[ids[k] - base];
}

// labels outside [0,nv) raise *err and are passed on as 0 so that the
// sort and the owner buckets stay inside the id range
__global__ void k_check_labels(i64 n, const i64 *__restrict__ labels, i64 nv,
                               i64 *__restrict__ out,
                               unsigned *__restrict__ err) {
    for (i64 v = blockIdx.x * (i64)blockDim.x + threadIdx.x; v < n;
         v += (i64)gridDim.x * blockDim.x) {
        const i64 l = labels[v];
        const bool bad = l < 0 || l >= nv;
        if (bad) *err = 1u;
        out[v] = bad ? 0 : l;
    }
}

__global__ void k_mark_owned(i64 n, const i64 *__restrict__ ids, i64 base,
                             unsigned *__restrict__ used) {
    for (i64 k = blockIdx.x * (i64)blockDim.x + threadIdx.x; k < n;
         k += (i64)gridDim.x * blockDim.x)
        used[ids[k] - base] = 1u;
}

__global__ void k_dense_ids(i64 n, const unsigned *__restrict__ rank,
                            i64 offset, i64 *__restrict__ dense) {
    for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < n;
         i += (i64)gridDim.x * blockDim.x)
        dense[i] = offset + (i64)rank[i];
}

// k_coarse_keys over one rank's slice: rows are local (map holds the lnv
// owned vertices), a tail inside [base,bound) reads map directly and a
// remote one the value fetched for it (ghost_ids sorted unique, ghost_map
// aligned with it)
__global__ __launch_bounds__(256) void k_coarse_keys_dist(
    i64 lnv, i64 lne, const i64 *__restrict__ xadj,
    const i64 *__restrict__ tails, i64 base, i64 bound,
    const i64 *__restrict__ map, const i64 *__restrict__ ghost_ids,
    i64 nghost, const i64 *__restrict__ ghost_map, int shift,
    u64 *__restrict__ keys) {
    const int lane = threadIdx.x & 63;
    const i64 wave = (blockIdx.x * (i64)blockDim.x + threadIdx.x) >> 6;
    const i64 nwaves = ((i64)gridDim.x * blockDim.x) >> 6;
    for (i64 e0 = wave * 64; e0 < lne; e0 += nwaves * 64) {
        const i64 e1 = e0 + 63 < lne ? e0 + 63 : lne - 1;
        const i64 r0 = row_of(xadj, 0, lnv - 1, e0);
        const i64 r1 = row_of(xadj, r0, lnv - 1, e1);
        const i64 e = e0 + lane;
        if (e <= e1) {
            const i64 r = row_of(xadj, r0, r1, e);
            const i64 t = tails[e];
            i64 ct;
            if (t >= base && t < bound) {
                ct = map[t - base];
            } else {
                i64 lo = 0, hi = nghost - 1; // t is in ghost_ids
                while (lo < hi) {
                    const i64 mid = (lo + hi) >> 1;
                    if (ghost_ids[mid] < t) lo = mid + 1;
                    else hi = mid;
                }
                ct = ghost_map[lo];
            }
            keys[e] = ((u64)map[r] << shift) | (u64)ct;
        }
    }
}

} // namespace

void mv_sort_unique_ids(hipStream_t st, int64_t n, const int64_t *d_ids,
                        int bits, mv_unique_ids *out) {
    *out = mv_unique_ids{};
    out->n = n;
    out->d_uniq.reserve(n); // never null, n == 0 included
    out->d_perm.reserve(n);
    out->d_run.reserve(n);
    if (n == 0) return;
    DevBuf<i64> sorted(n);
    DevBuf<unsigned> iota(n), head(n + 1), pos(n + 1);
    DevBuf<char> tmp; // freed at return, after the synchronising read
    k_iota<<<grid_for(n), 256, 0, st>>>(n, iota.get());
    cub_sort_pairs(tmp, st, d_ids, sorted.get(), iota.get(),
                   out->d_perm.get(), n, bits);
    k_id_heads<<<grid_for(n + 1), 256, 0, st>>>(n, sorted, head);
    mv_exclusive_sum_u32(st, head, pos, n + 1);
    k_id_runs<<<grid_for(n), 256, 0, st>>>(n, sorted, head, pos, out->d_run,
                                           out->d_uniq);
    out->nuniq = read_back(pos + n, st);
}

void mv_scatter_unique(hipStream_t st, const mv_unique_ids *u,
                       const int64_t *d_vals, int64_t *d_out) {
    if (u->n == 0) return;
    k_scatter_unique<<<grid_for(u->n), 256, 0, st>>>(u->n, u->d_perm,
                                                     u->d_run, d_vals, d_out);
}

void mv_lower_bounds(hipStream_t st, const uint64_t *d_sorted, int64_t n,
                     const uint64_t *h_keys, int m, int64_t *h_out) {
    DevBuf<uint64_t> d_keys(m);
    DevBuf<i64> d_out(m);
    HIP_CHECK(hipMemcpyAsync(d_keys, h_keys, 8 * (size_t)m,
                             hipMemcpyHostToDevice, st));
    lower_bounds_device(st, d_sorted, n, d_keys.get(), m, d_out.get());
    HIP_CHECK(hipMemcpyAsync(h_out, d_out, 8 * (size_t)m,
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
}

void mv_gather_owned(hipStream_t st, int64_t n, const int64_t *d_ids,
                     int64_t base, const int64_t *d_table, int64_t *d_out) {
    if (n == 0) return;
    k_gather_owned<<<grid_for(n), 256, 0, st>>>(n, d_ids, base, d_table,
                                                d_out);
}

void mv_check_labels(hipStream_t st, int64_t n, const int64_t *d_labels,
                     int64_t nv, int64_t *d_out, unsigned *d_err) {
    if (n == 0) return;
    k_check_labels<<<grid_for(n), 256, 0, st>>>(n, d_labels, nv, d_out,
                                                d_err);
}

void mv_mark_owned(hipStream_t st, int64_t n, const int64_t *d_ids,
                   int64_t base, unsigned *d_used) {
    if (n == 0) return;
    k_mark_owned<<<grid_for(n), 256, 0, st>>>(n, d_ids, base, d_used);
}

void mv_exclusive_sum_u32(hipStream_t st, const unsigned *d_in,
                          unsigned *d_out, int64_t n) {
    DevBuf<char> tmp;
    cub_exclusive_sum(tmp, st, d_in, d_out, n);
    HIP_CHECK(hipStreamSynchronize(st)); // tmp dies with this scope
}

void mv_dense_ids(hipStream_t st, int64_t n, const unsigned *d_rank,
                  int64_t offset, int64_t *d_dense) {
    if (n == 0) return;
    k_dense_ids<<<grid_for(n), 256, 0, st>>>(n, d_rank, offset, d_dense);
}

void mv_coarse_keys_dist(hipStream_t st, int64_t lnv, int64_t lne,
                         const int64_t *d_xadj, const int64_t *d_tails,
                         int64_t base, int64_t bound, const int64_t *d_map,
                         const int64_t *d_ghost_ids, int64_t nghost,
                         const int64_t *d_ghost_map, int shift,
                         uint64_t *d_keys) {
    if (lne == 0) return;
    k_coarse_keys_dist<<<grid_for(lne), 256, 0, st>>>(
        lnv, lne, d_xadj, d_tails, base, bound, d_map, d_ghost_ids, nghost,
        d_ghost_map, shift, (u64 *)d_keys);
}

void mv_coarse_rows(hipStream_t st, int64_t row0, int64_t nrows,
                    int64_t nruns, int shift, const uint64_t *d_run_key,
                    int64_t *d_cxadj, int64_t *d_ctails) {
    k_coarse_rows<<<grid_for(std::max(nruns, nrows + 1)), 256, 0, st>>>(
        row0, nrows, nruns, shift, (const u64 *)d_run_key, d_cxadj, d_ctails);
}
