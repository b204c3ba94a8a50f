// coarsen.h — internal seam between coarsen.hip (the community-aggregation
// kernels) and engine.hip (the multi-phase driver). Not part of the C-ABI.
#ifndef MINIVITE_COARSEN_H
#define MINIVITE_COARSEN_H

#include <cstdint>

#include <hip/hip_runtime.h>

// Device-resident result of one aggregation. d_map is always set; the CSR
// arrays stay null when the call stopped after renumbering.
struct mv_coarse_dev {
    int64_t nc = 0;            // coarse vertices
    int64_t ne = 0;            // coarse directed edges (distinct pairs)
    int64_t *d_map = nullptr;  // nv: fine vertex -> dense coarse id
    int64_t *d_xadj = nullptr; // nc+1
    int64_t *d_tails = nullptr; // ne, ascending within a row
    double *d_w = nullptr;      // ne
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

void mv_coarse_dev_free(mv_coarse_dev *c);

#endif
