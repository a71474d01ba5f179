// mq_scan.hip — the library's device prefix scan (mqi::scan_*_exclusive, mq_common.h).

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mq_common.h"
#include "mq_device.h"
#include "mq_radix.h"

namespace {

using namespace mqi;

// ---------------------------------------------------------------------------
// exclusive scan: Tin[n] -> u64[n] (reduce-then-scan over 4096-element tiles)
// ---------------------------------------------------------------------------
template <typename Tin>
__global__ __launch_bounds__(kTPB) void k_tile_sum(const Tin* in, uint64_t n, u64* sums) {
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile;
    u64 acc = 0;
    Tin v[kScanItems];  // all loads in flight first (clamped index, no branch)
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        const uint64_t i = base + (uint64_t)k * kTPB + threadIdx.x;
        v[k] = in[i < n ? i : n - 1];
    }
#pragma unroll
    for (int k = 0; k < kScanItems; k++)
        if (base + (uint64_t)k * kTPB + threadIdx.x < n) acc += (u64)v[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    __shared__ u64 ws[kTPB / 64];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// in and out may alias (every element is read into LDS before any is written).
template <typename Tin, typename Tout = u64>
__global__ __launch_bounds__(kTPB) void k_tile_scan(const Tin* in, Tout* out, uint64_t n,
                                                    const u64* offs) {
    __shared__ u64 tile[kScanTile];
    __shared__ u64 ws[kTPB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile;
    {
        Tin x[kScanItems];  // all loads in flight first (clamped index, no branch)
#pragma unroll
        for (int k = 0; k < kScanItems; k++) {
            const uint64_t i = base + (uint64_t)k * kTPB + tid;
            x[k] = in[i < n ? i : n - 1];
        }
#pragma unroll
        for (int k = 0; k < kScanItems; k++)
            tile[k * kTPB + tid] = base + (uint64_t)k * kTPB + tid < n ? (u64)x[k] : 0ull;
    }
    __syncthreads();
    u64 v[kScanItems];
    u64 acc = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        v[k] = tile[tid * kScanItems + k];
        acc += v[k];
    }
    const u64 incl = wave_incl_scan(acc, lane);
    if (lane == 63) ws[wave] = incl;
    __syncthreads();
    u64 run = incl - acc + (offs ? offs[blockIdx.x] : 0ull);
    for (int w = 0; w < wave; w++) run += ws[w];
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        tile[tid * kScanItems + k] = run;
        run += v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        const uint64_t i = base + (uint64_t)k * kTPB + tid;
        if (i < n) out[i] = (Tout)tile[k * kTPB + tid];
    }
}

// u64 elements of scratch needed by scan_exclusive(n).
uint64_t scan_scratch_elems(uint64_t n) {
    uint64_t total = 0;
    while (n > (uint64_t)kScanTile) {
        n = ceil_div(n, kScanTile);
        total += n;
    }
    return total + 1;
}

template <typename Tin, typename Tout = u64>
int scan_exclusive(const Tin* in, Tout* out, uint64_t n, u64* scratch, hipStream_t st) {
    if (n == 0) return MQ_OK;
    if (n <= (uint64_t)kScanTile) {
        hipLaunchKernelGGL((k_tile_scan<Tin, Tout>), dim3(1), dim3(kTPB), 0, st, in, out, n,
                           (const u64*)nullptr);
        LAUNCHCHK("k_tile_scan");
        return MQ_OK;
    }
    const uint64_t nb = ceil_div(n, kScanTile);
    hipLaunchKernelGGL(k_tile_sum<Tin>, dim3((uint32_t)nb), dim3(kTPB), 0, st, in, n, scratch);
    LAUNCHCHK("k_tile_sum");
    int rc = scan_exclusive<u64, u64>(scratch, scratch, nb, scratch + nb, st);
    if (rc) return rc;
    hipLaunchKernelGGL((k_tile_scan<Tin, Tout>), dim3((uint32_t)nb), dim3(kTPB), 0, st, in, out, n,
                       (const u64*)scratch);
    LAUNCHCHK("k_tile_scan");
    return MQ_OK;
}

}  // namespace

namespace mqi {
uint64_t scan_u32_scratch_elems(uint64_t n) { return scan_scratch_elems(n); }
int scan_u32_exclusive(const uint32_t* in, unsigned long long* out, uint64_t n,
                       unsigned long long* scratch, hipStream_t st) {
    return scan_exclusive<uint32_t>(in, out, n, scratch, st);
}
int scan_u32_exclusive_u32(const uint32_t* in, uint32_t* out, uint64_t n, unsigned long long* scratch,
                           hipStream_t st) {
    return scan_exclusive<uint32_t, uint32_t>(in, out, n, scratch, st);
}
int scan_u64_exclusive(const unsigned long long* in, unsigned long long* out, uint64_t n,
                       unsigned long long* scratch, hipStream_t st) {
    return scan_exclusive<u64>(in, out, n, scratch, st);
}
}  // namespace mqi

