// mq_rsort.hip — the stable LSD radix sort (mqi::radix_sort_pairs, radix_sort_lsd_index,
// mq_common.h): the sorted-index build's (mq_isort.hip) and the join's sorted-runs fallback.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mq_common.h"
#include "mq_device.h"
#include "mq_radix.h"

namespace {

using namespace mqi;

// ---------------------------------------------------------------------------
// stable LSD radix sort of packed words {key ^ 2^31 (low 32), value (high 32)},
// 8-bit digits. Per tile of TPB x IT words (8192): an LDS histogram (k_sortw_hist), an exclusive
// scan over (digit, tile), then a scatter that ranks equal digits with 8 wave
// ballots (stable) and stages the tile in LDS, so every digit run leaves the block
// as contiguous stores. (Element-by-element scatter measured 0.5 TB/s at 1e9 rows.)
// FIRST: the words are built from the int32 keys (and values, or row ids).
// LAST : the sorted words are written split into key and value arrays.
// ---------------------------------------------------------------------------
template <bool FIRST>
__device__ __forceinline__ u64 sort_word(const int* c1, const int* p1, const u64* in, uint64_t i) {
    if constexpr (FIRST) {
        const uint32_t v = p1 ? (uint32_t)p1[i] : (uint32_t)i;
        return (u64)((uint32_t)c1[i] ^ 0x80000000u) | ((u64)v << 32);
    } else {
        return in[i];
    }
}

template <bool FIRST, int TPB, int IT>
__global__ __launch_bounds__(TPB) void k_sortw_hist(const int* __restrict__ c1, const u64* __restrict__ in,
                                                    uint64_t n, int shift, uint32_t kmin,
                                                    uint32_t* __restrict__ hist, uint32_t ntiles) {
    constexpr uint32_t kTile = TPB * IT;
    __shared__ uint32_t h[kRadix];
    if (threadIdx.x < kRadix) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t tile = xcd_tile(blockIdx.x, gridDim.x);
    const uint64_t base = (uint64_t)tile * kTile;
    // all of the lane's items are loaded before any is counted (indices clamped,
    // no branch), so the loads share one round trip instead of one each; the words
    // are read once, nontemporal (1.72 -> 1.62 ms per pass over 8 GB at 1e9 rows)
    uint32_t key[IT];
#pragma unroll
    for (int k = 0; k < IT; k++) {
        const uint64_t i = base + (uint64_t)k * TPB + threadIdx.x;
        const uint64_t ic = i < n ? i : n - 1;
        key[k] = (FIRST ? ((uint32_t)__builtin_nontemporal_load(c1 + ic) ^ 0x80000000u)
                        : (uint32_t)__builtin_nontemporal_load(in + ic)) - kmin;
    }
#pragma unroll
    for (int k = 0; k < IT; k++)
        if (base + (uint64_t)k * TPB + threadIdx.x < n) atomicAdd(&h[(key[k] >> shift) & 0xFF], 1u);
    __syncthreads();
    if (threadIdx.x < kRadix) hist[(uint64_t)threadIdx.x * ntiles + tile] = h[threadIdx.x];
}

// The same histogram from the digit bytes the previous scatter wrote (1 B per row
// instead of the 8-byte words): one 16-byte load per thread covers its 16 rows.
template <int TPB, int IT>
__global__ __launch_bounds__(TPB) void k_sortw_hist_bytes(const uint8_t* __restrict__ dig, uint64_t n,
                                                          uint32_t* __restrict__ hist, uint32_t ntiles) {
    constexpr uint32_t kTile = TPB * IT;
    __shared__ uint32_t h[kRadix];
    if (threadIdx.x < kRadix) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t tile = xcd_tile(blockIdx.x, gridDim.x);
    const uint64_t base = (uint64_t)tile * kTile + (uint64_t)threadIdx.x * IT;
    static_assert(IT == 16, "one 16-byte load per thread");
    if (base + IT <= n) {
        typedef unsigned int v4u __attribute__((ext_vector_type(4)));
        const v4u w = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(dig + base));
        const uint32_t x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            atomicAdd(&h[x[k] & 0xFF], 1u);
            atomicAdd(&h[(x[k] >> 8) & 0xFF], 1u);
            atomicAdd(&h[(x[k] >> 16) & 0xFF], 1u);
            atomicAdd(&h[x[k] >> 24], 1u);
        }
    } else {
        for (uint64_t i = base; i < n && i < base + IT; i++) atomicAdd(&h[dig[i]], 1u);
    }
    __syncthreads();
    if (threadIdx.x < kRadix) hist[(uint64_t)threadIdx.x * ntiles + tile] = h[threadIdx.x];
}

// LAST: 0 = packed words to out, 1 = split into kout (flipped keys) / vout,
// 2 = an index: kout as int32 values (key ^ 2^31 undone), pout as size_t rows.
template <bool FIRST, int LAST, int TPB, int IT>
__global__ __launch_bounds__(TPB) void k_sortw_scatter(const int* __restrict__ c1, const int* __restrict__ p1,
                                                        const u64* __restrict__ in, uint64_t n, int shift,
                                                        uint32_t kmin, const u64* __restrict__ goff, uint32_t ntiles,
                                                        u64* __restrict__ out, uint32_t* __restrict__ kout,
                                                        uint32_t* __restrict__ vout, u64* __restrict__ pout,
                                                        uint8_t* __restrict__ dig) {
    constexpr int kW = TPB / 64;
    constexpr uint32_t kTile = TPB * IT;
    __shared__ uint32_t wcnt[kW][kRadix];
    __shared__ uint32_t loff[kRadix];
    __shared__ u64 gofs[kRadix];
    __shared__ u64 stage[kTile];
    __shared__ uint32_t wsum[kRadix / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int x = tid; x < kW * kRadix; x += TPB) (&wcnt[0][0])[x] = 0;
    const uint32_t tile = xcd_tile(blockIdx.x, gridDim.x);
    if (tid < kRadix) gofs[tid] = goff[(uint64_t)tid * ntiles + tile];
    __syncthreads();
    const uint64_t tile0 = (uint64_t)tile * kTile;
    const uint64_t seg = tile0 + (uint64_t)wave * (64 * IT);
    u64 el[IT];
    uint32_t dr[IT];
    // all items loaded first (indices clamped, no branch): one round trip, not one
    // per item (the ranking's ballots kept the compiler from hoisting the loads)
#pragma unroll
    for (int k = 0; k < IT; k++) {
        const uint64_t i = seg + (uint64_t)k * 64 + lane;
        el[k] = sort_word<FIRST>(c1, p1, in, i < n ? i : n - 1);
    }
#pragma unroll
    for (int k = 0; k < IT; k++) {
        const uint64_t i = seg + (uint64_t)k * 64 + lane;
        const bool valid = i < n;
        const uint32_t d = (((uint32_t)el[k] - kmin) >> shift) & 0xFF;
        const u64 peers = match_any8(d, __ballot(valid));
        const uint32_t lt = lanes_below(peers);
        const uint32_t cur = wcnt[wave][d];
        __builtin_amdgcn_wave_barrier();
        if (valid && lt == 0) wcnt[wave][d] = cur + (uint32_t)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
        dr[k] = valid ? ((d << 16) | (cur + lt)) : 0xFFFFFFFFu;
    }
    __syncthreads();
    // per digit (thread tid < 256): prefix over the waves, then the tile-local
    // exclusive scan of the digit totals (waves 0-3)
    uint32_t tot = 0, incl = 0;
    if (tid < kRadix) {
#pragma unroll
        for (int w = 0; w < kW; w++) {
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
#pragma unroll
    for (int k = 0; k < IT; k++) {
        if (dr[k] != 0xFFFFFFFFu) {
            const uint32_t d = dr[k] >> 16, r = dr[k] & 0xFFFF;
            stage[loff[d] + wcnt[wave][d] + r] = el[k];
        }
    }
    __syncthreads();
    const uint64_t tn = n - tile0 < (uint64_t)kTile ? n - tile0 : (uint64_t)kTile;
#pragma unroll
    for (int k = 0; k < IT; k++) {
        const uint32_t e = (uint32_t)(k * TPB + tid);
        if (e < tn) {
            const u64 v = stage[e];
            const uint32_t d = (((uint32_t)v - kmin) >> shift) & 0xFF;
            const u64 dst = gofs[d] + (e - loff[d]);
            if constexpr (LAST == 1) {
                kout[dst] = (uint32_t)v;
                vout[dst] = (uint32_t)(v >> 32);
            } else if constexpr (LAST == 2) {
                if (kout) kout[dst] = (uint32_t)v ^ 0x80000000u;
                if (pout) pout[dst] = v >> 32;
            } else {
                out[dst] = v;
                if (dig) dig[dst] = (uint8_t)(((uint32_t)v - kmin) >> (shift + 8));  // the next pass's digit
            }
        }
    }
}

}  // namespace

namespace mqi {

template <int TPB, int IT>
int radix_sort_tiles(const int* c1, const int* p1, uint64_t n, int mode, uint32_t kmin, int npass, uint32_t* kout,
                     uint32_t* vout, u64* pout, hipStream_t st);

int radix_sort_run(const int* c1, const int* p1, uint64_t n, int mode, uint32_t* kout, uint32_t* vout,
                   u64* pout, hipStream_t st) {
    // (A onesweep form, decoupled look-back instead of a histogram pass per pass, measured
    // slower and was removed in round 6: 1e9-row index 27.9 vs 22.3 ms, its scatter passes
    // 6.3-7.1 ms against 3.7-4.4 + 1.6 ms of histogram; right after launch every resident
    // tile walked back over ~2000 unfinished predecessors through cross-XCD status loads.)
    // tiles of 512 x 16 words: 18.7 ms for the 1e9-row index, against 21.6 with
    // 256 x 16 (digit runs of 16 words leave the block as 128-B pieces), 25.9 with
    // 1024 x 8 and 22.3 with 512 x 8 (tools/sorttpb_cmd.sh)
    return radix_sort_tiles<kSortTPB, kSortItems>(c1, p1, n, mode, 0, 4, kout, vout, pout, st);
}

// npass 8-bit digits of (key ^ 2^31) - kmin, lowest first (1 <= npass <= 4): a key
// range of at most 8 * npass bits sorts in npass passes.
template <int TPB, int IT>
int radix_sort_tiles(const int* c1, const int* p1, uint64_t n, int mode, uint32_t kmin, int npass, uint32_t* kout,
                     uint32_t* vout, u64* pout, hipStream_t st) {
    constexpr uint64_t kTile = (uint64_t)TPB * IT;
    u64 *w0 = nullptr, *w1 = nullptr, *hscan = nullptr, *scratch = nullptr;
    uint32_t* hist = nullptr;
    uint8_t* dig = nullptr;  // the next pass's digit of every row, written by the scatter
    const uint64_t ntiles = ceil_div(n, kTile);
    const uint64_t nh = ntiles * kRadix;
    auto done = [&](int rc) {
        pool_free_on(w0, st);
        pool_free_on(w1, st);
        pool_free_on(hist, st);
        pool_free_on(hscan, st);
        pool_free_on(scratch, st);
        pool_free_on(dig, st);
        return rc;
    };
    if (npass < 1 || npass > 4) return set_err(MQ_EINVAL, "sort: %d passes", npass);
    w0 = (u64*)pool_alloc(n * 8);
    const bool use_dig = npass > 1;
    if (use_dig) dig = (uint8_t*)pool_alloc(n + 16);
    w1 = (u64*)pool_alloc(n * 8);
    hist = (uint32_t*)pool_alloc(nh * 4);
    hscan = (u64*)pool_alloc(nh * 8);
    scratch = (u64*)pool_alloc(scan_u32_scratch_elems(nh) * 8);
    if (!w0 || !w1 || !hist || !hscan || !scratch || (use_dig && !dig))
        return done(set_err(MQ_ENOMEM, "sort: buffers (%llu rows)", (unsigned long long)n));
    const dim3 g((uint32_t)ntiles), b(TPB);
    const uint32_t nt = (uint32_t)ntiles;
    for (int pass = 0; pass < npass; pass++) {
        const int shift = 8 * pass;
        const bool first = pass == 0, last = pass == npass - 1;
        uint8_t* dnext = last ? nullptr : dig;
        if (first)
            hipLaunchKernelGGL((k_sortw_hist<true, TPB, IT>), g, b, 0, st, c1, nullptr, n, shift, kmin, hist, nt);
        else if (use_dig)
            hipLaunchKernelGGL((k_sortw_hist_bytes<TPB, IT>), g, b, 0, st, dig, n, hist, nt);
        else
            hipLaunchKernelGGL((k_sortw_hist<false, TPB, IT>), g, b, 0, st, nullptr, w0, n, shift, kmin, hist, nt);
        int rc = scan_u32_exclusive(hist, hscan, nh, scratch, st);
        if (rc) return done(rc);
        if (first && !last)
            hipLaunchKernelGGL((k_sortw_scatter<true, 0, TPB, IT>), g, b, 0, st, c1, p1, nullptr, n, shift, kmin, hscan,
                               nt, w1, nullptr, nullptr, nullptr, dnext);
        else if (!last)
            hipLaunchKernelGGL((k_sortw_scatter<false, 0, TPB, IT>), g, b, 0, st, nullptr, nullptr, w0, n, shift, kmin,
                               hscan, nt, w1, nullptr, nullptr, nullptr, dnext);
        else if (mode == 1 && first)
            hipLaunchKernelGGL((k_sortw_scatter<true, 1, TPB, IT>), g, b, 0, st, c1, p1, nullptr, n, shift, kmin, hscan,
                               nt, nullptr, kout, vout, nullptr, nullptr);
        else if (mode == 1)
            hipLaunchKernelGGL((k_sortw_scatter<false, 1, TPB, IT>), g, b, 0, st, nullptr, nullptr, w0, n, shift, kmin,
                               hscan, nt, nullptr, kout, vout, nullptr, nullptr);
        else if (first)
            hipLaunchKernelGGL((k_sortw_scatter<true, 2, TPB, IT>), g, b, 0, st, c1, p1, nullptr, n, shift, kmin, hscan,
                               nt, nullptr, kout, nullptr, pout, nullptr);
        else
            hipLaunchKernelGGL((k_sortw_scatter<false, 2, TPB, IT>), g, b, 0, st, nullptr, nullptr, w0, n, shift, kmin,
                               hscan, nt, nullptr, kout, nullptr, pout, nullptr);
        if (hipGetLastError() != hipSuccess) return done(set_err(MQ_EHIP, "sort: launch"));
        u64* t = w0;
        w0 = w1;
        w1 = t;
    }
    // the temporaries go back to the pool only after the passes have run
    if (hipStreamSynchronize(st) != hipSuccess) return done(set_err(MQ_EHIP, "sort: sync"));
    return done(MQ_OK);
}

int radix_sort_pairs(const int* c1, const int* p1, uint64_t n, uint32_t** keys_out,
                     uint32_t** vals_out, hipStream_t st, const DevState*) {
    uint32_t* ko = (uint32_t*)pool_alloc(n ? n * 4 : 16);
    uint32_t* vo = (uint32_t*)pool_alloc(n ? n * 4 : 16);
    if (!ko || !vo) {
        pool_free_on(ko, st);
        pool_free_on(vo, st);
        return set_err(MQ_ENOMEM, "sort: outputs (%llu rows)", (unsigned long long)n);
    }
    int rc = n ? radix_sort_run(c1, p1, n, 1, ko, vo, nullptr, st) : MQ_OK;
    if (rc) {
        pool_free_on(ko, st);
        pool_free_on(vo, st);
        return rc;
    }
    *keys_out = ko;
    *vals_out = vo;
    return MQ_OK;
}

int radix_sort_lsd_index(const int* col, uint64_t n, uint32_t kmin, int npass, int32_t* values, uint64_t* positions,
                         hipStream_t st) {
    return n ? radix_sort_tiles<kSortTPB, kSortItems>(col, nullptr, n, 2, kmin, npass,
                                                      reinterpret_cast<uint32_t*>(values), nullptr,
                                                      reinterpret_cast<u64*>(positions), st)
             : MQ_OK;
}

}  // namespace mqi

