// cub_util.h — the one place hipCUB is called. Each wrapper asks for the
// temporary-storage size, grows the caller's `tmp` to it, runs on `st` and
// checks the return code; n == 0 launches nothing. `tmp` is the caller's so
// that a caller which may not allocate (halo_prep: a hipFree would
// serialise the overlapped pipeline) passes a buffer it sized beforehand
// (cub_presize_sort_unique); one-shot callers pass a local one and keep it
// alive until the stream has drained. Item counts are below 2^31.
#ifndef MINIVITE_CUB_UTIL_H
#define MINIVITE_CUB_UTIL_H

#include <hipcub/hipcub.hpp>

#include "device_util.h"

// call(storage, bytes) is one hipCUB entry point with its arguments bound
template <class F> void cub_run(DevBuf<char> &tmp, F call) {
    size_t bytes = 0;
    HIP_CHECK(call(nullptr, bytes));
    tmp.reserve((i64)bytes);
    HIP_CHECK(call(tmp.get(), bytes));
}

// stable ascending radix sort over the low `bits` key bits
template <class K>
void cub_sort_keys(DevBuf<char> &tmp, hipStream_t st, const K *in, K *out,
                   i64 n, int bits) {
    if (n == 0) return;
    cub_run(tmp, [&](void *t, size_t &b) {
        return hipcub::DeviceRadixSort::SortKeys(t, b, in, out, n, 0, bits,
                                                 st);
    });
}

template <class K, class V>
void cub_sort_pairs(DevBuf<char> &tmp, hipStream_t st, const K *kin, K *kout,
                    const V *vin, V *vout, i64 n, int bits) {
    if (n == 0) return;
    cub_run(tmp, [&](void *t, size_t &b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, kin, kout, vin, vout,
                                                  n, 0, bits, st);
    });
}

template <class K, class V>
void cub_sort_pairs_descending(DevBuf<char> &tmp, hipStream_t st,
                               const K *kin, K *kout, const V *vin, V *vout,
                               i64 n, int bits) {
    if (n == 0) return;
    cub_run(tmp, [&](void *t, size_t &b) {
        return hipcub::DeviceRadixSort::SortPairsDescending(
            t, b, kin, kout, vin, vout, n, 0, bits, st);
    });
}

// distinct values of a sorted array; *d_num (device) = their count, 0 for
// n == 0
template <class T>
void cub_unique(DevBuf<char> &tmp, hipStream_t st, const T *in, T *out,
                i64 *d_num, i64 n) {
    if (n == 0) {
        HIP_CHECK(hipMemsetAsync(d_num, 0, sizeof(i64), st));
        return;
    }
    cub_run(tmp, [&](void *t, size_t &b) {
        return hipcub::DeviceSelect::Unique(t, b, in, out, d_num, n, st);
    });
}

// Grow tmp to what cub_sort_keys and cub_unique of n i64 ids take, running
// neither: later calls with no more than n ids then never allocate.
inline void cub_presize_sort_unique(DevBuf<char> &tmp, i64 n, int bits) {
    size_t a = 0, b = 0;
    const i64 *in = nullptr; // the argument types of the two wrappers
    i64 *out = nullptr;
    HIP_CHECK(
        hipcub::DeviceRadixSort::SortKeys(nullptr, a, in, out, n, 0, bits));
    HIP_CHECK(hipcub::DeviceSelect::Unique(nullptr, b, in, out, out, n));
    tmp.reserve((i64)std::max(a, b));
}

// the flagged elements in order; *d_num (device) = their count, 0 for
// n == 0
template <class T>
void cub_select_flagged(DevBuf<char> &tmp, hipStream_t st, const T *in,
                        const unsigned char *flags, T *out, i64 *d_num,
                        i64 n) {
    if (n == 0) {
        HIP_CHECK(hipMemsetAsync(d_num, 0, sizeof(i64), st));
        return;
    }
    cub_run(tmp, [&](void *t, size_t &b) {
        return hipcub::DeviceSelect::Flagged(t, b, in, flags, out, d_num, n,
                                             st);
    });
}

template <class T>
void cub_inclusive_sum(DevBuf<char> &tmp, hipStream_t st, const T *in, T *out,
                       i64 n) {
    if (n == 0) return;
    cub_run(tmp, [&](void *t, size_t &b) {
        return hipcub::DeviceScan::InclusiveSum(t, b, in, out, n, st);
    });
}

template <class T>
void cub_exclusive_sum(DevBuf<char> &tmp, hipStream_t st, const T *in, T *out,
                       i64 n) {
    if (n == 0) return;
    cub_run(tmp, [&](void *t, size_t &b) {
        return hipcub::DeviceScan::ExclusiveSum(t, b, in, out, n, st);
    });
}

#endif
