// mq_keyset.hip — a set of int32 keys on the device as a bitmap over its span (DESIGN.md
// §3.17): the build side of select_where_in (WHERE k [NOT] IN (SELECT ...)). The probes,
// mq_semi_positions and mq_semi_agg, are in mq_where.hip.
//
// The set is one bit per value of [lo, hi]: bit (uint32)(key - lo), in 32-bit words, the
// bitmap rounded up to 16 bytes and zeroed (512 MiB at the full int32 span). Without given
// bounds lo and hi are the column's min and max (mq_reduce, one more read of the keys).
//
//   k_keyset_build : streams the column like k_scan (contiguous chunks from mqi::geometry,
//                    nt dwordx4 loads, kUnroll tiles in flight, dword loads for a column off a
//                    16-byte boundary, a ragged tail row by row) and sets the keys' bits with a
//                    global atomic OR whose result is not used. The word is read first and the
//                    atomic skipped when the bit is set already: bits only go from 0 to 1, so a
//                    stale read costs one redundant atomic and never a wrong bit, and a column
//                    of one hot key does not queue n atomics on one address. That read is a
//                    relaxed device-scope load, served by L2 where the atomics land (a line in
//                    a CU's vector cache would stay stale for as long as it stays there). Keys
//                    outside given bounds are counted, not set.
//   k_keyset_count : the bits that are set = COUNT(DISTINCT).
// The build synchronises: the host reads the bounds, the count and the out-of-bounds count.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>

#include "mq_common.h"
#include "mq_device.h"
#include "mq_scan_common.h"
#include "mq_where_common.h"

namespace {

using namespace mqi;
using u64 = unsigned long long;

template <bool VEC>
__global__ __launch_bounds__(kTPB, 8) void k_keyset_build(const int32_t* __restrict__ keys, uint64_t n,
                                                          uint64_t rows_per_block, uint32_t lo, uint32_t wm1,
                                                          uint32_t* __restrict__ bits, u64* __restrict__ hdr) {
    const int tid = threadIdx.x, lane = tid & 63;
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;

    uint32_t bad = 0;
    auto put = [&](int k) {
        const uint32_t d = (uint32_t)k - lo;
        if (d > wm1) {
            bad++;
            return;
        }
        uint32_t* w = bits + (d >> 5);
        const uint32_t m = 1u << (d & 31u);
        if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m)) atomicOr(w, m);
    };
    auto put4 = [&](int4 v) {
        put(v.x);
        put(v.y);
        put(v.z);
        put(v.w);
    };

    uint64_t t = start;
    for (; t + (uint64_t)kUnroll * kTileRows <= end; t += (uint64_t)kUnroll * kTileRows) {
        int4 v[kUnroll];
        const int32_t* __restrict__ p = keys + t + (uint64_t)tid * 4;
#pragma unroll
        for (int u = 0; u < kUnroll; u++) v[u] = load4_nt<VEC>(p + (uint64_t)u * kTileRows);
#pragma unroll
        for (int u = 0; u < kUnroll; u++) put4(v[u]);
    }
    for (; t + kTileRows <= end; t += kTileRows) put4(load4_nt<VEC>(keys + t + (uint64_t)tid * 4));
    if (t < end) {  // the column's ragged tile
        const uint64_t row = t + (uint64_t)tid * 4;
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (row + e < end) put(keys[row + e]);
    }
    const u64 wb = wave_sum_u64((u64)bad);
    if (lane == 0 && wb) atomicAdd(hdr + 1, wb);
}

// hdr[0] += the set bits of the bitmap's vec16 16-byte pieces.
__global__ __launch_bounds__(kTPB) void k_keyset_count(const uint4* __restrict__ bits, uint64_t vec16,
                                                       u64* __restrict__ hdr) {
    uint32_t c = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x; i < vec16; i += (uint64_t)gridDim.x * kTPB) {
        const uint4 q = bits[i];
        c += (uint32_t)(__popc(q.x) + __popc(q.y) + __popc(q.z) + __popc(q.w));
    }
    const u64 wc = wave_sum_u64((u64)c);
    if ((threadIdx.x & 63) == 0 && wc) atomicAdd(hdr, wc);
}

}  // namespace

extern "C" {

int mq_keyset_build(const int32_t* d_keys, uint64_t n1, int has_bounds, int32_t lo, int32_t hi, mq_keyset** out,
                    mq_keyset_info* h_info, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (out) *out = nullptr;
    if (!out) return set_err(MQ_EINVAL, "mq_keyset_build: NULL out");
    if (n1 >= (1ull << 31)) return set_err(MQ_EINVAL, "mq_keyset_build: n1 >= 2^31");
    if (n1 && (!d_keys || (reinterpret_cast<uintptr_t>(d_keys) & 3u)))
        return set_err(MQ_EINVAL, "mq_keyset_build: keys NULL or not 4-byte aligned");
    if (has_bounds && lo > hi) return set_err(MQ_EINVAL, "mq_keyset_build: bounds [%d, %d] are empty", lo, hi);
    hipStream_t st = (hipStream_t)stream;
    int dev = -1;
    if ((rc = current_device(&dev))) return rc;
    mq_keyset* ks = new (std::nothrow) mq_keyset();
    if (!ks) return set_err(MQ_ENOMEM, "mq_keyset_build: out of host memory");
    ks->dev = dev;
    ks->lo = 0;
    ks->hi = -1;
    if (n1 == 0) {
        if (h_info) *h_info = mq_keyset_info{ks->lo, ks->hi, 0, 0};
        *out = ks;
        return MQ_OK;
    }
    // the partials of mq_reduce, its aggregate, and {distinct, keys out of bounds}
    char* ws = static_cast<char*>(pool_alloc(partial_bytes() + sizeof(mq_agg) + 2 * sizeof(u64)));
    if (!ws) {
        delete ks;
        return set_err(MQ_ENOMEM, "mq_keyset_build: workspace allocation failed");
    }
    auto fail = [&](int code) {
        (void)hipStreamSynchronize(st);  // nothing queued here still uses the buffers
        pool_free(ks->bits);
        pool_free(ws);
        delete ks;
        return code;
    };
    mq_agg* d_agg = reinterpret_cast<mq_agg*>(ws + partial_bytes());
    u64* d_hdr = reinterpret_cast<u64*>(d_agg + 1);
    if (!has_bounds) {  // one more read of the keys
        mq_agg a = {};
        rc = mq_reduce(d_keys, n1, d_agg, ws, partial_bytes(), stream);
        if (!rc && hipMemcpyAsync(&a, d_agg, sizeof a, hipMemcpyDeviceToHost, st) != hipSuccess)
            rc = set_err(MQ_EHIP, "mq_keyset_build: bounds download failed");
        if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = set_err(MQ_EHIP, "mq_keyset_build: stream failed");
        if (rc) return fail(rc);
        lo = a.min;
        hi = a.max;
    }
    const uint32_t wm1 = (uint32_t)hi - (uint32_t)lo;
    const uint64_t vec16 = ((uint64_t)wm1 + 128) / 128;  // (span + 127) / 128
    ks->bytes = vec16 * 16;
    ks->bits = static_cast<uint32_t*>(pool_alloc(ks->bytes));
    if (!ks->bits) return fail(set_err(MQ_ENOMEM, "mq_keyset_build: %llu bytes of bitmap", (u64)ks->bytes));
    if (hipMemsetAsync(ks->bits, 0, ks->bytes, st) != hipSuccess || hipMemsetAsync(d_hdr, 0, 2 * sizeof(u64), st) != hipSuccess)
        return fail(set_err(MQ_EHIP, "mq_keyset_build: memset failed"));
    const bool vec = aligned16(d_keys);
    uint32_t g;
    uint64_t rpb;
    geometry(s, n1, vec ? reinterpret_cast<const void*>(&k_keyset_build<true>) : reinterpret_cast<const void*>(&k_keyset_build<false>),
             &g, &rpb, (uint64_t)kUnroll * kTileRows);
    if (vec)
        hipLaunchKernelGGL((k_keyset_build<true>), dim3(g), dim3(kTPB), 0, st, d_keys, n1, rpb, (uint32_t)lo, wm1, ks->bits, d_hdr);
    else
        hipLaunchKernelGGL((k_keyset_build<false>), dim3(g), dim3(kTPB), 0, st, d_keys, n1, rpb, (uint32_t)lo, wm1, ks->bits, d_hdr);
    hipLaunchKernelGGL(k_keyset_count, dim3(stream_grid(s, vec16)), dim3(kTPB), 0, st, reinterpret_cast<const uint4*>(ks->bits),
                       (uint64_t)vec16, d_hdr);
    u64 h[2] = {0, 0};
    if (hipGetLastError() != hipSuccess) return fail(set_err(MQ_EHIP, "launch of k_keyset_build / k_keyset_count failed"));
    if (hipMemcpyAsync(h, d_hdr, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail(set_err(MQ_EHIP, "mq_keyset_build: header download failed"));
    if (h[1]) return fail(set_err(MQ_EINVAL, "mq_keyset_build: %llu keys outside the bounds [%d, %d]", h[1], lo, hi));
    pool_free(ws);
    ks->lo = lo;
    ks->hi = hi;
    ks->distinct = h[0];
    if (h_info) *h_info = mq_keyset_info{lo, hi, ks->distinct, ks->bytes};
    *out = ks;
    return MQ_OK;
}

int mq_keyset_free(mq_keyset* ks) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!ks) return MQ_OK;
    pool_free(ks->bits);
    delete ks;
    return MQ_OK;
}

}  // extern "C"
