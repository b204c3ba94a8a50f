// coarsen.h — internal seam between coarsen.hip (the community-aggregation
// kernels) and multiphase.hip (the multi-phase driver). Not part of the
// C-ABI. The result structs own their device memory (DevBuf members, so
// they are move-only): whoever holds one returns on any path without
// clean-up.
#ifndef MINIVITE_COARSEN_H
#define MINIVITE_COARSEN_H

#include "device_util.h"

// Device-resident result of one aggregation. d_map is always set; the CSR
// arrays stay null when the call stopped after renumbering.
struct mv_coarse_dev {
    int64_t nc = 0;          // coarse vertices
    int64_t ne = 0;          // coarse directed edges (distinct pairs)
    DevBuf<int64_t> d_map;   // nv: fine vertex -> dense coarse id
    DevBuf<int64_t> d_xadj;  // nc+1
    DevBuf<int64_t> d_tails; // ne, ascending within a row
    DevBuf<double> d_w;      // ne
};

// Aggregate the single-rank device CSR (xadj/tails; d_w null = unit
// weights) by d_labels (nv labels, each in [0,nv)). With
// stop_if_identity, a labelling that merges nothing (nc == nv) returns
// after the renumbering with the CSR arrays null. Synchronises `st`.
// Returns 0, or non-zero with a message on stderr (label out of range,
// lne >= 2^31).
int mv_coarsen_device(hipStream_t st, int64_t nv, int64_t lne,
                      const int64_t *d_xadj, const int64_t *d_tails,
                      const double *d_w, const int64_t *d_labels,
                      bool stop_if_identity, mv_coarse_dev *out);

// ---- building blocks shared with the distributed aggregation ----
// Everything below is transport-free: multiphase.hip strings the pieces
// together across the exchange seam. Each call works on `st`; the ones
// that return host values or device allocations synchronise it.

// One (key, summed weight) per distinct key, keys ascending.
struct mv_key_runs {
    int64_t n = 0;
    DevBuf<uint64_t> d_key; // neither is null after the call
    DevBuf<double> d_w;
};

// Stable radix sort of n (key, weight) pairs over the low `bits` key bits,
// run heads, and the fixed-order run reduction (<= 32 entries left to
// right by one thread, longer runs by one block's fixed tree): no
// floating-point atomics, bit-identical run to run. d_w null = every
// weight is 1 and a run's weight is its length. 0 <= n < 2^31 - 1; the
// inputs are not modified.
void mv_sort_reduce_keys(hipStream_t st, int64_t n, const uint64_t *d_keys,
                         const double *d_w, int bits, mv_key_runs *out);

// Sorted distinct values of n non-negative ids (< 2^bits) plus the way
// back: input position d_perm[i] holds the id of run d_run[i].
struct mv_unique_ids {
    int64_t n = 0, nuniq = 0;
    DevBuf<int64_t> d_uniq; // nuniq ids, ascending
    DevBuf<unsigned> d_perm; // n: sorted position -> input position
    DevBuf<unsigned> d_run;  // n: sorted position -> index into d_uniq
};
void mv_sort_unique_ids(hipStream_t st, int64_t n, const int64_t *d_ids,
                        int bits, mv_unique_ids *out);
// d_out[input position] = d_vals[index of its id in d_uniq]
void mv_scatter_unique(hipStream_t st, const mv_unique_ids *u,
                       const int64_t *d_vals, int64_t *d_out);

// h_out[j] = first index of d_sorted[0,n) whose value is >= h_keys[j]
// (owner buckets of sorted ids or keys); host in, host out.
void mv_lower_bounds(hipStream_t st, const uint64_t *d_sorted, int64_t n,
                     const uint64_t *h_keys, int m, int64_t *h_out);

// owner side: d_out[k] = d_table[d_ids[k] - base]
void mv_gather_owned(hipStream_t st, int64_t n, const int64_t *d_ids,
                     int64_t base, const int64_t *d_table, int64_t *d_out);
// renumbering: copy labels (one outside [0,nv) raises *d_err and becomes
// 0), mark the owned labels in use, dense id = offset + rank in use
void mv_check_labels(hipStream_t st, int64_t n, const int64_t *d_labels,
                     int64_t nv, int64_t *d_out, unsigned *d_err);
void mv_mark_owned(hipStream_t st, int64_t n, const int64_t *d_ids,
                   int64_t base, unsigned *d_used);
void mv_exclusive_sum_u32(hipStream_t st, const unsigned *d_in,
                          unsigned *d_out, int64_t n); // 1 <= n < 2^31
void mv_dense_ids(hipStream_t st, int64_t n, const unsigned *d_rank,
                  int64_t offset, int64_t *d_dense);

// (map[row] << shift) | coarse id of the tail, per local edge of a slice
// owning [base,bound): local tails read d_map, remote ones d_ghost_map at
// their position in the sorted distinct d_ghost_ids.
void mv_coarse_keys_dist(hipStream_t st, int64_t lnv, int64_t lne,
                         const int64_t *d_xadj, const int64_t *d_tails,
                         int64_t base, int64_t bound, const int64_t *d_map,
                         const int64_t *d_ghost_ids, int64_t nghost,
                         const int64_t *d_ghost_map, int shift,
                         uint64_t *d_keys);
// offsets of rows row0 .. row0+nrows (nrows+1 values, relative to the
// first run) and the tails of sorted distinct keys
void mv_coarse_rows(hipStream_t st, int64_t row0, int64_t nrows,
                    int64_t nruns, int shift, const uint64_t *d_run_key,
                    int64_t *d_cxadj, int64_t *d_ctails);

#endif
