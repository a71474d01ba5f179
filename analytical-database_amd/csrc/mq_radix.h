// mq_radix.h — internal: the tile constants and wave / tile scan helpers shared by the
// device scan (mq_scan.hip), the LSD radix sort (mq_rsort.hip) and the join's window
// partition (mq_join.hip, mq_join_part.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mqi {

typedef unsigned long long u64;

constexpr int kTPB = 256;
constexpr int kScanItems = 16;
constexpr int kScanTile = kTPB * kScanItems;  // 4096
constexpr int kSortItems = 16;  // words per thread of a sort tile (8 and 32 measured slower)
constexpr int kRadix = 256;
constexpr int kSortTPB = 512;  // sort tile = kSortTPB x kSortItems words (radix_sort_tiles)

__device__ __forceinline__ u64 wave_incl_scan(u64 v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 y = __shfl_up(v, off, 64);
        if (lane >= off) v += y;
    }
    return v;
}

inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// After a tile's items are ranked per wave (wcnt[w][d] = wave w's count of digit d):
// wcnt[w][d] becomes the count of d in the waves before w, loff[d] the tile-local start
// of digit d. Threads 0..255 (waves 0-3) own the digits; every thread takes the barriers.
template <int TPB>
__device__ __forceinline__ void tile_digit_offsets(uint32_t (*wcnt)[kRadix], uint32_t* loff, uint32_t* wsum,
                                                   int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t tot = 0, incl = 0;
    if (tid < kRadix) {
#pragma unroll
        for (int w = 0; w < TPB / 64; w++) {
            const uint32_t c = wcnt[w][tid];
            wcnt[w][tid] = tot;
            tot += c;
        }
        incl = tot;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(incl, off, 64);
            if (lane >= off) incl += y;
        }
        if (lane == 63) wsum[wave] = incl;
    }
    __syncthreads();
    if (tid < kRadix) {
        uint32_t excl = incl - tot;
        for (int w = 0; w < wave; w++) excl += wsum[w];
        loff[tid] = excl;
    }
    __syncthreads();
}

// Exclusive scan of a tile's 256 digit counts (threads 0..255 own the digits; every
// thread takes the barriers): loff[d] = the tile-local start of digit d.
__device__ __forceinline__ void digit_scan(const uint32_t* cnt, uint32_t* loff, uint32_t* wsum, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t c = 0, incl = 0;
    if (tid < kRadix) {
        c = cnt[tid];
        incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(incl, off, 64);
            if (lane >= off) incl += y;
        }
        if (lane == 63) wsum[wave] = incl;
    }
    __syncthreads();
    if (tid < kRadix) {
        uint32_t ex = incl - c;
        for (int w = 0; w < wave; w++) ex += wsum[w];
        loff[tid] = ex;
    }
    __syncthreads();
}

}  // namespace mqi
