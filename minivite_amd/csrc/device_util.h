// device_util.h — device plumbing every translation unit shares: error
// check, the one owner of device / pinned memory, and the small device and
// host primitives of the engine and the aggregation. No RCCL, no hipCUB
// (that is cub_util.h). Not part of the C-ABI.
#ifndef MINIVITE_DEVICE_UTIL_H
#define MINIVITE_DEVICE_UTIL_H

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include <hip/hip_runtime.h>

#define HIP_CHECK(x)                                                         \
    do {                                                                      \
        hipError_t _e = (x);                                                  \
        if (_e != hipSuccess) {                                               \
            std::fprintf(stderr, "HIP error %s at %s:%d: %s\n",               \
                         hipGetErrorString(_e), __FILE__, __LINE__, #x);      \
            std::abort();                                                     \
        }                                                                     \
    } while (0)

using i64 = int64_t;

// first index in the sorted a[0,n) whose value is >= key (i64 or u64 keys)
template <class K>
__device__ __forceinline__ i64 dev_lower_bound(const K *a, i64 n, K key) {
    i64 lo = 0, hi = n;
    while (lo < hi) {
        i64 mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void atomic_add_i64(i64 *p, i64 v) {
    atomicAdd(reinterpret_cast<unsigned long long *>(p),
              static_cast<unsigned long long>(v));
}

inline int grid_for(i64 n, int block = 256, int cap = 2048) {
    i64 g = (n + block - 1) / block;
    return (int)std::min<i64>(std::max<i64>(g, 1), cap);
}

// bits that hold every value below n (at least one): the radix-sort width
// of ids in [0,n) and the shift that packs two of them into one key
inline int ceil_log2(i64 n) {
    int b = 1;
    while ((1ll << b) < n) b++;
    return b;
}

using clk = std::chrono::steady_clock;
inline double ms_since(clk::time_point t0) {
    return std::chrono::duration<double, std::milli>(clk::now() - t0).count();
}

// Move-only owner of one device (hipMalloc) or pinned host (hipHostMalloc)
// allocation. reserve() is grow-only and does NOT preserve contents; it
// floors n at one element so the pointer is never null once reserved.
template <class T, bool PINNED = false> struct DevBuf {
    T *ptr = nullptr;
    i64 cap = 0; // elements
    DevBuf() = default;
    explicit DevBuf(i64 n) { reserve(n); }
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
    T *get() const { return ptr; }
    operator T *() const { return ptr; }
};
template <class T> using PinBuf = DevBuf<T, true>;

// one value read back from the device on st; returns once it has arrived
template <class T> T read_back(const T *d, hipStream_t st) {
    T h;
    HIP_CHECK(hipMemcpyAsync(&h, d, sizeof(T), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return h;
}

// Kernels two translation units launch. Templates, so that a unit which
// launches none of them carries none of them.
template <class T> __global__ void k_iota(i64 n, T *__restrict__ out) {
    for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < n;
         i += (i64)gridDim.x * blockDim.x)
        out[i] = (T)i;
}

// out[j] = first index of sorted[0,n) whose value is >= keys[j], j < m:
// with a partition's m = nranks+1 boundaries as the keys, the per-owner
// buckets of a sorted id (or packed key) array
template <class K>
__global__ void k_lower_bounds(const K *__restrict__ sorted, i64 n,
                               const K *__restrict__ keys, int m,
                               i64 *__restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) out[j] = dev_lower_bound(sorted, n, keys[j]);
}
template <class K>
void lower_bounds_device(hipStream_t st, const K *d_sorted, i64 n,
                         const K *d_keys, int m, i64 *d_out) {
    k_lower_bounds<<<(m + 63) / 64, 64, 0, st>>>(d_sorted, n, d_keys, m,
                                                 d_out);
}

#endif
