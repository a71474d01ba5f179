// mq_keymap.hip — a map from an int32 primary key to an int32 attribute on the device
// (DESIGN.md §3.18): the build side of group_aggregate_join (GROUP BY an attribute of a
// dimension joined N:1 on its key) and, with mq_keymap_lookup, the materialised N:1 join.
// The fused probe, k_group_join_dense, is in mq_group.hip.
//
// One representation for every span [lo, hi] of the keys:
//   the bitmap of mq_keyset_build (one bit per value of the span, built by that code, so that
//   mq_keymap_keyset is an ordinary key set);
//   a rank directory, one u64 per 32 keys of the span (per bitmap word, the 16-byte padding
//   included): low half the bitmap word, high half the set bits of all earlier words, an
//   exclusive prefix below 2^31;
//   the attributes in key order, attr_by_rank[n1].
// A lookup is d = (uint32)(key - lo) <= hi - lo, one 8-byte load e = dir[d >> 5], a bit test,
// rank = (e >> 32) + popc(low(e) & ((1 << (d & 31)) - 1)) and one 4-byte load attr_by_rank[rank].
// At the full int32 span that is 512 MiB of bitmap, 1 GiB of directory and 4 * n1 bytes.
//
//   k_keymap_word_sums : the set bits of each chunk of bitmap words (a fixed grid of at most
//                        kMapBlocks chunks of whole 256-word steps, mq_keymap_geometry).
//   k_keymap_dir       : each block sums the chunks below its own, then walks its chunk in
//                        256-word steps: a block scan of the words' popcounts, carried from
//                        step to step, gives every word's prefix; the entry leaves with one
//                        8-byte store.
//   k_keymap_place     : attr_by_rank[rank(keys[i])] = attrs[i], grid-stride. The keys are a
//                        primary key (the build refuses distinct != n1), so every rank is
//                        written once and the result does not depend on the order.
//   k_keymap_lookup    : grid-stride, keys read directly or through positions.
// The build synchronises: the host reads the key set's count and the attributes' range.

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <new>

#include "mq_common.h"
#include "mq_device.h"
#include "mq_scan_common.h"
#include "mq_where_common.h"

namespace {

using namespace mqi;
using u64 = unsigned long long;

constexpr uint32_t kMapBlocks = 2048;  // chunks of the directory's prefix pass

// Bitmap words (32 keys each) of a span of `span` values, the 16-byte padding included.
uint64_t span_words(uint64_t span) { return (span + 127) / 128 * 4; }

void dir_chunks(uint64_t words, uint32_t* blocks, uint64_t* chunk) { chunks(words, kTPB, kMapBlocks, blocks, chunk); }

__global__ __launch_bounds__(kTPB) void k_keymap_word_sums(const uint32_t* __restrict__ bits, uint64_t words, uint64_t chunk,
                                                           uint32_t* __restrict__ csum) {
    __shared__ uint32_t s_w[kWaves];
    const uint64_t w0 = (uint64_t)blockIdx.x * chunk;
    const uint64_t w1 = w0 + chunk < words ? w0 + chunk : words;
    uint32_t c = 0;
    for (uint64_t w = w0 + threadIdx.x; w < w1; w += kTPB) c += (uint32_t)__popc(bits[w]);
    const uint32_t total = block_sum(c, s_w);
    if (threadIdx.x == 0) csum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kTPB) void k_keymap_dir(const uint32_t* __restrict__ bits, uint64_t words, uint64_t chunk,
                                                     const uint32_t* __restrict__ csum, u64* __restrict__ dir) {
    __shared__ uint32_t s_w[kWaves];
    uint32_t below = 0;
    for (uint32_t i = threadIdx.x; i < blockIdx.x; i += kTPB) below += csum[i];
    uint32_t base = block_sum(below, s_w);
    const uint64_t w0 = (uint64_t)blockIdx.x * chunk;
    const uint64_t w1 = w0 + chunk < words ? w0 + chunk : words;
    for (uint64_t s = w0; s < w1; s += kTPB) {  // block-uniform trip count
        const uint64_t w = s + threadIdx.x;
        const uint32_t word = w < w1 ? bits[w] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_scan((uint32_t)__popc(word), s_w, &total);
        if (w < w1) dir[w] = ((u64)(base + ex) << 32) | word;
        base += total;
    }
}

__global__ __launch_bounds__(kTPB) void k_keymap_place(MapArgs m, const int32_t* __restrict__ attrs, uint64_t n1,
                                                       int32_t* __restrict__ by_rank) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x; i < n1; i += stride) {
        const uint32_t d = (uint32_t)m.key[i] - m.lo;
        const u64 e = map_entry(m, d);
        // every key is in the set it was built from; its rank is below the n1 set bits
        if (map_hit(e, d)) by_rank[map_rank(e, d)] = attrs[i];
    }
}

__global__ __launch_bounds__(kTPB) void k_keymap_lookup(MapArgs m, bool empty, const int32_t* __restrict__ pos, uint64_t k,
                                                        int32_t missing, int32_t* __restrict__ attr_out,
                                                        uint8_t* __restrict__ hit_out) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x; i < k; i += stride) {
        const int32_t key = m.key[pos ? (uint32_t)pos[i] : i];
        const uint32_t d = (uint32_t)key - m.lo;
        const u64 e = empty ? 0ull : map_entry(m, d);
        const bool hit = map_hit(e, d);
        attr_out[i] = hit ? m.attr[map_rank(e, d)] : missing;
        if (hit_out) hit_out[i] = hit ? 1 : 0;
    }
}

void release(mq_keymap* km) {
    if (!km) return;
    mq_keyset_free(km->ks);
    pool_free(km->dir);
    pool_free(km->attr);
    delete km;
}

}  // namespace

extern "C" {

size_t mq_keymap_bytes(uint64_t span, uint64_t n1) {
    const uint64_t words = span_words(span);
    return (size_t)(words * 4 + words * 8 + n1 * 4);
}

void mq_keymap_geometry(uint64_t span, uint32_t* prefix_blocks, uint64_t* prefix_chunk_words) {
    uint32_t b;
    uint64_t c;
    dir_chunks(span_words(span), &b, &c);
    if (prefix_blocks) *prefix_blocks = b;
    if (prefix_chunk_words) *prefix_chunk_words = c;
}

int mq_keymap_build(const int32_t* d_keys, const int32_t* d_attrs, uint64_t n1, int has_bounds, int32_t lo, int32_t hi,
                    mq_keymap** out, mq_keymap_info* h_info, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (out) *out = nullptr;
    if (!out) return set_err(MQ_EINVAL, "mq_keymap_build: NULL out");
    if (n1 >= (1ull << 31)) return set_err(MQ_EINVAL, "mq_keymap_build: n1 >= 2^31");
    if (n1 && (!d_keys || (reinterpret_cast<uintptr_t>(d_keys) & 3u)))
        return set_err(MQ_EINVAL, "mq_keymap_build: keys NULL or not 4-byte aligned");
    if (n1 && (!d_attrs || (reinterpret_cast<uintptr_t>(d_attrs) & 3u)))
        return set_err(MQ_EINVAL, "mq_keymap_build: attributes NULL or not 4-byte aligned");
    if (has_bounds && lo > hi) return set_err(MQ_EINVAL, "mq_keymap_build: bounds [%d, %d] are empty", lo, hi);
    hipStream_t st = (hipStream_t)stream;
    mq_keymap* km = new (std::nothrow) mq_keymap();
    if (!km) return set_err(MQ_ENOMEM, "mq_keymap_build: out of host memory");
    km->attr_lo = INT_MAX;
    km->attr_hi = INT_MIN;
    mq_keyset_info ki = {};
    if ((rc = mq_keyset_build(d_keys, n1, has_bounds, lo, hi, &km->ks, &ki, stream))) {  // synchronises
        delete km;
        return rc;
    }
    if (n1 == 0) {
        if (h_info) *h_info = mq_keymap_info{0, -1, INT_MAX, INT_MIN, 0, 0};
        *out = km;
        return MQ_OK;
    }
    if (ki.distinct != n1) {
        release(km);
        return set_err(MQ_EINVAL, "mq_keymap_build: the keys are not a primary key: %llu of %llu repeat an earlier key",
                       (u64)(n1 - ki.distinct), (u64)n1);
    }
    const uint64_t words = km->ks->bytes / 4;
    uint32_t blocks;
    uint64_t chunk;
    dir_chunks(words, &blocks, &chunk);
    km->n1 = n1;
    km->dir = static_cast<u64*>(pool_alloc(words * 8));
    km->attr = static_cast<int32_t*>(pool_alloc(n1 * 4));
    // the chunks' sums, then mq_reduce's partials and its aggregate
    const size_t csum_bytes = ((size_t)kMapBlocks * 4 + 15) & ~(size_t)15;
    char* ws = static_cast<char*>(pool_alloc(csum_bytes + partial_bytes() + sizeof(mq_agg)));
    auto fail = [&](int code) {
        (void)hipStreamSynchronize(st);  // nothing queued here still uses the buffers
        pool_free(ws);
        release(km);
        return code;
    };
    if (!km->dir || !km->attr || !ws) return fail(set_err(MQ_ENOMEM, "mq_keymap_build: allocation failed"));
    km->bytes = km->ks->bytes + words * 8 + n1 * 4;
    uint32_t* csum = reinterpret_cast<uint32_t*>(ws);
    mq_agg* d_agg = reinterpret_cast<mq_agg*>(ws + csum_bytes + partial_bytes());
    const MapArgs m = {d_keys, km->dir, km->attr, (uint32_t)ki.lo, (uint32_t)ki.hi - (uint32_t)ki.lo};
    hipLaunchKernelGGL(k_keymap_word_sums, dim3(blocks), dim3(kTPB), 0, st, km->ks->bits, words, chunk, csum);
    hipLaunchKernelGGL(k_keymap_dir, dim3(blocks), dim3(kTPB), 0, st, km->ks->bits, words, chunk, csum, km->dir);
    hipLaunchKernelGGL(k_keymap_place, dim3(stream_grid(s, n1)), dim3(kTPB), 0, st, m, d_attrs, n1, km->attr);
    if (hipGetLastError() != hipSuccess) return fail(set_err(MQ_EHIP, "launch of k_keymap_dir / k_keymap_place failed"));
    mq_agg a = {};
    if ((rc = mq_reduce(d_attrs, n1, d_agg, ws + csum_bytes, partial_bytes(), stream))) return fail(rc);
    if (hipMemcpyAsync(&a, d_agg, sizeof a, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail(set_err(MQ_EHIP, "mq_keymap_build: attribute range download failed"));
    pool_free(ws);
    km->attr_lo = a.min;
    km->attr_hi = a.max;
    if (h_info) *h_info = mq_keymap_info{ki.lo, ki.hi, km->attr_lo, km->attr_hi, n1, km->bytes};
    *out = km;
    return MQ_OK;
}

const mq_keyset* mq_keymap_keyset(const mq_keymap* km) { return km ? km->ks : nullptr; }

int mq_keymap_lookup(const mq_keymap* km, const int32_t* d_keys, const int32_t* d_pos, uint64_t k, int32_t missing,
                     int32_t* d_attr_out, uint8_t* d_hit_out, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!km) return set_err(MQ_EINVAL, "mq_keymap_lookup: NULL key map");
    if (k >= (1ull << 31)) return set_err(MQ_EINVAL, "mq_keymap_lookup: k >= 2^31");
    if (k && (!d_keys || !d_attr_out || (reinterpret_cast<uintptr_t>(d_keys) & 3u) || (reinterpret_cast<uintptr_t>(d_pos) & 3u) ||
              (reinterpret_cast<uintptr_t>(d_attr_out) & 3u)))
        return set_err(MQ_EINVAL, "mq_keymap_lookup: keys or output NULL, or a pointer not 4-byte aligned");
    int dev = -1;
    if ((rc = current_device(&dev))) return rc;
    if (dev != km->ks->dev) return set_err(MQ_EINVAL, "mq_keymap_lookup: the key map lives on device %d, the call runs on %d", km->ks->dev, dev);
    if (k == 0) return MQ_OK;
    const bool empty = km->ks->lo > km->ks->hi;
    const MapArgs m = {d_keys, km->dir, km->attr, (uint32_t)km->ks->lo, empty ? 0u : (uint32_t)km->ks->hi - (uint32_t)km->ks->lo};
    hipLaunchKernelGGL(k_keymap_lookup, dim3(stream_grid(s, k)), dim3(kTPB), 0, (hipStream_t)stream, m, empty, d_pos, k, missing,
                       d_attr_out, d_hit_out);
    LAUNCHCHK("k_keymap_lookup");
    return MQ_OK;
}

int mq_keymap_free(mq_keymap* km) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    release(km);
    return MQ_OK;
}

}  // extern "C"
