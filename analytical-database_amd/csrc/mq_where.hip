// mq_where.hip — one-pass conjunctive range select over up to 8 columns.
//
// P columns of n int32 rows and P ranges: row i matches when low_c <= col_c[i] < high_c holds
// for every c (either bound optional, as select_column defines one range). Two forms:
//   positions: d_payload ? d_payload[i] : i of every matching row, ascending i, and their
//              number K: what the chain select -> fetch -> select_result -> ... returns;
//   aggregate: {count, int64 sum, min, max} of d_val[i] over the matching rows.
// The reference has no such operator (its DSL spells a conjunction as that chain); the
// semantics are restated in numpy by tests/wherecases.py. Integer operations only: every
// grid, predicate order and alignment gives the same bytes.
//
// The host folds each range into Pred's one unsigned compare; a range that matches every
// int32 drops out (its column is never read) and an empty one ends the call before any
// launch. Pointers and folded ranges travel by value in the kernel arguments.
//
// Both forms stream like k_scan: 256-thread blocks on contiguous chunks from mqi::geometry,
// nt dwordx4 loads, kWhU tiles (1024 rows each) in flight per lane. Column 0 is read whole.
// After predicate c every wave tile (256 rows, 4 per lane) has a ballot of the lanes that
// still hold a surviving row. A lane loads its 16 bytes of column c + 1 only when one of the
// 8 lanes of its group does: 8 lanes x 16 B are one 128-byte line, the request size of this
// part, so a line in which predicates 0..c left no row is never requested, and a tile
// without a survivor issues nothing (wave-uniform). The loads of all tiles of the iteration
// are issued before the first is evaluated. The aggregate's value column is read under the
// same rule after the last predicate.
//
//   k_where_agg    : that stream; one Partial per block, folded by mq_combine_partials.
//   k_where_mask   : that stream; per wave tile the four ballots of its rows (word e, bit l:
//                    row 256 t + 4 l + e) and its match count.
//   (scan)         : the library's exclusive scan over the counts (reduce-then-scan).
//   k_where_expand : one block per 4096 rows. A row's output slot follows from the prefix of
//                    its wave tile and the ballots alone. The block's entries (row ids, or
//                    payload rows loaded where a bit is set) are gathered in LDS, placed so
//                    that LDS index and output address agree modulo 16 bytes, and leave as
//                    dwordx4 stores (k_dml_compact's shape).
// No kernel waits for another block.
//
// mq_semi_positions / mq_semi_agg put a key [NOT] IN set predicate behind
// the ranges in the same stream: k_semi_mask and k_semi_agg, further down, with the scan and
// k_where_expand shared. mq_star_positions puts up to four such predicates
// there, one per key map or key set of a star query's terms: k_star_mask, global bitmap only.

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "mq_common.h"
#include "mq_device.h"
#include "mq_scan_common.h"
#include "mq_where_common.h"

namespace {

using namespace mqi;
using u64 = unsigned long long;

constexpr int kWhU = 8;                        // tiles in flight per lane
constexpr int kWaveRows = 256;                 // rows of a wave tile
constexpr int kExpTile = 4096;                 // rows per expand block
constexpr int kExpWt = kExpTile / kWaveRows;   // its wave tiles

template <bool VEC>
__global__ __launch_bounds__(kTPB, 8) void k_where_mask(WhereArgs a, uint64_t n, uint64_t rows_per_block,
                                                        u64* __restrict__ bm, uint32_t* __restrict__ cnt) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;

    // The wave's 256 rows of the tile at row t: four ballot words and their count.
    auto put = [&](uint64_t t, uint32_t live) {
        const u64 w0 = __ballot(live & 1u), w1 = __ballot(live & 2u), w2 = __ballot(live & 4u), w3 = __ballot(live & 8u);
        const uint64_t wt = t / kWaveRows + (uint64_t)wave;
        if (lane < 4) bm[wt * 4 + lane] = lane == 0 ? w0 : lane == 1 ? w1 : lane == 2 ? w2 : w3;
        if (lane == 0) cnt[wt] = (uint32_t)(__popcll(w0) + __popcll(w1) + __popcll(w2) + __popcll(w3));
    };

    uint64_t t = start;
    for (; t + (uint64_t)kWhU * kTileRows <= end; t += (uint64_t)kWhU * kTileRows) {
        uint32_t live[kWhU];
        live_tiles<VEC, kWhU>(a, t + (uint64_t)tid * 4, lane, live);
#pragma unroll
        for (int u = 0; u < kWhU; u++) put(t + (uint64_t)u * kTileRows, live[u]);
    }
    for (; t + kTileRows <= end; t += kTileRows) {  // the chunk's tail, whole tiles
        uint32_t live[1];
        live_tiles<VEC, 1>(a, t + (uint64_t)tid * 4, lane, live);
        put(t, live[0]);
    }
    if (t < end) put(t, live_ragged(a, t + (uint64_t)tid * 4, end));  // block-uniform
}

// Output slots [pre[16 b], pre[16 b + 16)) from the rows of block b's 16 wave tiles.
// pre[w] = matches before wave tile w, for w in [0, nwt]; pre[nwt] = K.
template <bool PAY>
__global__ __launch_bounds__(kTPB) void k_where_expand(const u64* __restrict__ bm, const uint32_t* __restrict__ pre,
                                                       uint32_t nwt, uint64_t n, const int32_t* __restrict__ payload,
                                                       int32_t* __restrict__ out, u64* __restrict__ count) {
    __shared__ __attribute__((aligned(16))) int s_buf[kExpTile + 4];
    __shared__ u64 s_word[kExpWt * 4];
    __shared__ uint32_t s_pre[kExpWt + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t wt0 = blockIdx.x * kExpWt;
    if (tid < kExpWt * 4) {
        const uint32_t wt = wt0 + (uint32_t)tid / 4u;
        s_word[tid] = wt < nwt ? bm[(uint64_t)wt * 4 + ((uint32_t)tid & 3u)] : 0ull;
    }
    if (tid <= kExpWt) {
        const uint32_t w = wt0 + (uint32_t)tid;
        s_pre[tid] = pre[w < nwt ? w : nwt];
    }
    if (blockIdx.x == 0 && tid == 0) *count = (u64)pre[nwt];
    __syncthreads();
    const uint32_t p0 = s_pre[0];
    const uint32_t cnt = s_pre[kExpWt] - p0;
    if (cnt == 0) return;  // block-uniform
    int32_t* __restrict__ o = out + p0;  // the block's first entry
    const uint32_t al = (uint32_t)((reinterpret_cast<uintptr_t>(o) >> 2) & 3u);
    const bool pvec = PAY && (reinterpret_cast<uintptr_t>(payload) & 15u) == 0;
#pragma unroll
    for (int j = 0; j < kExpWt / kWaves; j++) {
        const int wl = j * kWaves + wave;
        const u64 w0 = s_word[wl * 4 + 0], w1 = s_word[wl * 4 + 1], w2 = s_word[wl * 4 + 2], w3 = s_word[wl * 4 + 3];
        const uint32_t nib = (uint32_t)((w0 >> lane) & 1ull) | ((uint32_t)((w1 >> lane) & 1ull) << 1) |
                             ((uint32_t)((w2 >> lane) & 1ull) << 2) | ((uint32_t)((w3 >> lane) & 1ull) << 3);
        if (nib == 0u) continue;
        // entries of the block before this lane's rows: < cnt <= kExpTile
        uint32_t k = al + (s_pre[wl] - p0) + lanes_below(w0) + lanes_below(w1) + lanes_below(w2) + lanes_below(w3);
        const uint64_t row = ((uint64_t)(wt0 + (uint32_t)wl)) * kWaveRows + (uint64_t)lane * 4;  // a set bit: row + e < n
        int e0 = (int)row, e1 = (int)row + 1, e2 = (int)row + 2, e3 = (int)row + 3;
        if constexpr (PAY) {
            if (pvec && row + 4 <= n) {
                const int4 q = load4_nt<true>(payload + row);
                e0 = q.x, e1 = q.y, e2 = q.z, e3 = q.w;
            } else {
                if (nib & 1u) e0 = payload[row + 0];
                if (nib & 2u) e1 = payload[row + 1];
                if (nib & 4u) e2 = payload[row + 2];
                if (nib & 8u) e3 = payload[row + 3];
            }
        }
        if (nib & 1u) s_buf[k++] = e0;
        if (nib & 2u) s_buf[k++] = e1;
        if (nib & 4u) s_buf[k++] = e2;
        if (nib & 8u) s_buf[k++] = e3;
    }
    __syncthreads();
    const uint32_t end = al + cnt;
    int32_t* base = o - al;  // base + q is 16-byte aligned for q % 4 == 0
    for (uint32_t q = 4u * (uint32_t)tid; q < end; q += 4u * kTPB) {
        if (q >= al && q + 4u <= end) {
            *reinterpret_cast<int4*>(base + q) = *reinterpret_cast<const int4*>(s_buf + q);
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4; e++)
                if (q + e >= al && q + e < end) base[q + e] = s_buf[q + e];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kTPB, 8) void k_where_agg(WhereArgs a, const int32_t* __restrict__ val, uint64_t n,
                                                       uint64_t rows_per_block, Partial* __restrict__ part) {
    __shared__ Partial sp[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;

    uint32_t cnt = 0;
    long long sum = 0;
    int mn = INT_MAX, mx = INT_MIN;
    auto fold1 = [&](bool p, int v) {
        cnt += (uint32_t)p;
        sum += p ? (long long)v : 0ll;
        mn = min(mn, p ? v : INT_MAX);
        mx = max(mx, p ? v : INT_MIN);
    };
    auto fold = [&](int4 v, uint32_t live) {
        fold1(live & 1u, v.x);
        fold1(live & 2u, v.y);
        fold1(live & 4u, v.z);
        fold1(live & 8u, v.w);
    };
    // U full tiles: the value rows of the lines that still hold a survivor
    auto tiles = [&](auto uc, uint64_t t) {
        constexpr int U = decltype(uc)::value;
        const uint64_t row = t + (uint64_t)tid * 4;
        uint32_t live[U];
        live_tiles<VEC, U>(a, row, lane, live);
        u64 b[U];
        int4 v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            b[u] = __ballot(live[u] != 0u);
            if (b[u] != 0 && line_live(b[u], lane)) v[u] = load4_nt<VEC>(val + row + (uint64_t)u * kTileRows);
        }
#pragma unroll
        for (int u = 0; u < U; u++)
            if (live[u] != 0u) fold(v[u], live[u]);
    };

    uint64_t t = start;
    for (; t + (uint64_t)kWhU * kTileRows <= end; t += (uint64_t)kWhU * kTileRows)
        tiles(std::integral_constant<int, kWhU>{}, t);
    for (; t + kTileRows <= end; t += kTileRows) tiles(std::integral_constant<int, 1>{}, t);
    if (t < end) {  // the column's ragged tile
        const uint64_t row = t + (uint64_t)tid * 4;
        const uint32_t live = live_ragged(a, row, end);
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (live & (1u << e)) fold1(true, val[row + e]);
    }

    const u64 wc = wave_sum_u64((u64)cnt);
    sum = wave_sum_i64(sum);
    mn = wave_min(mn);
    mx = wave_max(mx);
    if (lane == 0) sp[wave] = Partial{wc, sum, mn, mx, 0ull};
    __syncthreads();
    if (tid == 0) {
        Partial r = sp[0];
#pragma unroll
        for (int w = 1; w < kWaves; w++) {
            r.count += sp[w].count;
            r.sum += sp[w].sum;
            r.mn = min(r.mn, sp[w].mn);
            r.mx = max(r.mx, sp[w].mx);
        }
        part[blockIdx.x] = r;
    }
}

// ---- ranges AND key [NOT] IN set (mq_semi_positions, mq_semi_agg) ----
// The key column is read as "the next column" behind the ranges: only the 128-byte lines in
// which a row survived are requested, the set (mq_keyset.hip: one bit per value of its span)
// is looked up for surviving rows only, and live &= hit (anti: ~hit). All lookups of an
// iteration are issued before the first is used. LDSSET: the block first copies the whole
// bitmap into dynamic LDS (coalesced dwordx4; the bitmap is 16-byte padded) and looks up
// there; otherwise the bit's word is a plain cached load, so that the bitmap stays in L2 and
// the Infinity Cache while the columns pass by non-temporally.

extern __shared__ __attribute__((aligned(16))) uint32_t s_semi_set[];

template <bool LDSSET>
__device__ __forceinline__ void semi_stage(const SemiArgs& k) {
    if constexpr (LDSSET) {
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(k.bits);
        uint4* dst = reinterpret_cast<uint4*>(s_semi_set);
        for (uint32_t i = threadIdx.x; i < k.vec16; i += kTPB) dst[i] = src[i];
        __syncthreads();
    }
}

template <bool LDSSET>
__device__ __forceinline__ uint32_t semi_word(const SemiArgs& k, uint32_t w) {
    if constexpr (LDSSET) {
        return s_semi_set[w];
    } else {
        return k.bits[w];
    }
}

// The set's words for the lane's surviving rows (0 for a dead row or a key outside the span).
template <bool LDSSET>
__device__ __forceinline__ void semi_words(const SemiArgs& k, int4 v, uint32_t live, uint32_t (&w)[4]) {
    const uint32_t d0 = (uint32_t)v.x - k.lo, d1 = (uint32_t)v.y - k.lo, d2 = (uint32_t)v.z - k.lo, d3 = (uint32_t)v.w - k.lo;
    w[0] = w[1] = w[2] = w[3] = 0u;
    if ((live & 1u) && d0 <= k.wm1) w[0] = semi_word<LDSSET>(k, d0 >> 5);
    if ((live & 2u) && d1 <= k.wm1) w[1] = semi_word<LDSSET>(k, d1 >> 5);
    if ((live & 4u) && d2 <= k.wm1) w[2] = semi_word<LDSSET>(k, d2 >> 5);
    if ((live & 8u) && d3 <= k.wm1) w[3] = semi_word<LDSSET>(k, d3 >> 5);
}

__device__ __forceinline__ uint32_t semi_hits(const SemiArgs& k, int4 v, const uint32_t (&w)[4]) {
    return ((w[0] >> (((uint32_t)v.x - k.lo) & 31u)) & 1u) | (((w[1] >> (((uint32_t)v.y - k.lo) & 31u)) & 1u) << 1) |
           (((w[2] >> (((uint32_t)v.z - k.lo) & 31u)) & 1u) << 2) | (((w[3] >> (((uint32_t)v.w - k.lo) & 31u)) & 1u) << 3);
}

// live_tiles, then the key predicate on what is left.
template <bool VEC, bool LDSSET, int U>
__device__ __forceinline__ void semi_tiles(const WhereArgs& a, const SemiArgs& k, uint64_t row, int lane, uint32_t (&live)[U]) {
    live_tiles<VEC, U>(a, row, lane, live);
    int4 v[U];
    uint32_t w[U][4];
    const int32_t* __restrict__ p = k.key + row;
#pragma unroll
    for (int u = 0; u < U; u++) {
        const u64 b = __ballot(live[u] != 0u);
        v[u] = make_int4(0, 0, 0, 0);
        if (b != 0 && line_live(b, lane)) v[u] = load4_nt<VEC>(p + (uint64_t)u * kTileRows);
    }
#pragma unroll
    for (int u = 0; u < U; u++) semi_words<LDSSET>(k, v[u], live[u], w[u]);
#pragma unroll
    for (int u = 0; u < U; u++) live[u] &= semi_hits(k, v[u], w[u]) ^ k.flip;
}

// The ragged tile, row by row.
template <bool LDSSET>
__device__ __forceinline__ uint32_t semi_ragged(const WhereArgs& a, const SemiArgs& k, uint64_t row, uint64_t end) {
    uint32_t live = live_ragged(a, row, end);
#pragma unroll
    for (int e = 0; e < 4; e++) {
        if (!(live & (1u << e))) continue;
        const uint32_t d = (uint32_t)k.key[row + e] - k.lo;
        const uint32_t hit = d <= k.wm1 ? (semi_word<LDSSET>(k, d >> 5) >> (d & 31u)) & 1u : 0u;
        if (hit == (k.flip & 1u)) live &= ~(1u << e);
    }
    return live;
}

// k_where_mask's ballot words and counts, with the key predicate behind the ranges.
template <bool VEC, bool LDSSET>
__global__ __launch_bounds__(kTPB, 4) void k_semi_mask(WhereArgs a, SemiArgs k, uint64_t n, uint64_t rows_per_block,
                                                       u64* __restrict__ bm, uint32_t* __restrict__ cnt) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;
    semi_stage<LDSSET>(k);

    auto put = [&](uint64_t t, uint32_t live) {
        const u64 w0 = __ballot(live & 1u), w1 = __ballot(live & 2u), w2 = __ballot(live & 4u), w3 = __ballot(live & 8u);
        const uint64_t wt = t / kWaveRows + (uint64_t)wave;
        if (lane < 4) bm[wt * 4 + lane] = lane == 0 ? w0 : lane == 1 ? w1 : lane == 2 ? w2 : w3;
        if (lane == 0) cnt[wt] = (uint32_t)(__popcll(w0) + __popcll(w1) + __popcll(w2) + __popcll(w3));
    };

    uint64_t t = start;
    for (; t + (uint64_t)kWhU * kTileRows <= end; t += (uint64_t)kWhU * kTileRows) {
        uint32_t live[kWhU];
        semi_tiles<VEC, LDSSET, kWhU>(a, k, t + (uint64_t)tid * 4, lane, live);
#pragma unroll
        for (int u = 0; u < kWhU; u++) put(t + (uint64_t)u * kTileRows, live[u]);
    }
    for (; t + kTileRows <= end; t += kTileRows) {
        uint32_t live[1];
        semi_tiles<VEC, LDSSET, 1>(a, k, t + (uint64_t)tid * 4, lane, live);
        put(t, live[0]);
    }
    if (t < end) put(t, semi_ragged<LDSSET>(a, k, t + (uint64_t)tid * 4, end));  // block-uniform
}

// k_where_agg with the key predicate behind the ranges; the value column comes last.
template <bool VEC, bool LDSSET>
__global__ __launch_bounds__(kTPB, 4) void k_semi_agg(WhereArgs a, SemiArgs k, const int32_t* __restrict__ val, uint64_t n,
                                                      uint64_t rows_per_block, Partial* __restrict__ part) {
    __shared__ Partial sp[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;
    semi_stage<LDSSET>(k);

    uint32_t cnt = 0;
    long long sum = 0;
    int mn = INT_MAX, mx = INT_MIN;
    auto fold1 = [&](bool p, int v) {
        cnt += (uint32_t)p;
        sum += p ? (long long)v : 0ll;
        mn = min(mn, p ? v : INT_MAX);
        mx = max(mx, p ? v : INT_MIN);
    };
    auto fold = [&](int4 v, uint32_t live) {
        fold1(live & 1u, v.x);
        fold1(live & 2u, v.y);
        fold1(live & 4u, v.z);
        fold1(live & 8u, v.w);
    };
    auto tiles = [&](auto uc, uint64_t t) {
        constexpr int U = decltype(uc)::value;
        const uint64_t row = t + (uint64_t)tid * 4;
        uint32_t live[U];
        semi_tiles<VEC, LDSSET, U>(a, k, row, lane, live);
        u64 b[U];
        int4 v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            b[u] = __ballot(live[u] != 0u);
            if (b[u] != 0 && line_live(b[u], lane)) v[u] = load4_nt<VEC>(val + row + (uint64_t)u * kTileRows);
        }
#pragma unroll
        for (int u = 0; u < U; u++)
            if (live[u] != 0u) fold(v[u], live[u]);
    };

    uint64_t t = start;
    for (; t + (uint64_t)kWhU * kTileRows <= end; t += (uint64_t)kWhU * kTileRows)
        tiles(std::integral_constant<int, kWhU>{}, t);
    for (; t + kTileRows <= end; t += kTileRows) tiles(std::integral_constant<int, 1>{}, t);
    if (t < end) {  // the column's ragged tile
        const uint64_t row = t + (uint64_t)tid * 4;
        const uint32_t live = semi_ragged<LDSSET>(a, k, row, end);
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (live & (1u << e)) fold1(true, val[row + e]);
    }

    const u64 wc = wave_sum_u64((u64)cnt);
    sum = wave_sum_i64(sum);
    mn = wave_min(mn);
    mx = wave_max(mx);
    if (lane == 0) sp[wave] = Partial{wc, sum, mn, mx, 0ull};
    __syncthreads();
    if (tid == 0) {
        Partial r = sp[0];
#pragma unroll
        for (int w = 1; w < kWaves; w++) {
            r.count += sp[w].count;
            r.sum += sp[w].sum;
            r.mn = min(r.mn, sp[w].mn);
            r.mx = max(r.mx, sp[w].mx);
        }
        part[blockIdx.x] = r;
    }
}

// ---- ranges AND every km / ks term of a star query (mq_star_positions) ----
// k_semi_mask with one key predicate per term, in the order given: before each term the tiles
// are balloted again, only the surviving 128-byte lines of the term's column are requested, and
// the bitmap word is loaded for surviving rows only (a plain cached load; for a key map the
// map's own key set bitmap, not its directory). The global bitmap only: there is no LDS form.
// `s` holds the filtering terms alone; none at all leaves the ranges (or, without any, every row).

template <bool VEC, int U>
__device__ __forceinline__ void star_tiles(const WhereArgs& a, const StarArgs& s, uint64_t row, int lane, uint32_t (&live)[U]) {
    live_tiles<VEC, U>(a, row, lane, live);
    for (int j = 0; j < s.nterms; j++) {
        const StarTerm& tm = s.t[j];
        int4 v[U];
        uint32_t w[U][4];
        u64 any = 0;
        const int32_t* __restrict__ p = tm.col + row;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const u64 b = __ballot(live[u] != 0u);
            any |= b;
            v[u] = make_int4(0, 0, 0, 0);
            if (b != 0 && line_live(b, lane)) v[u] = load4_nt<VEC>(p + (uint64_t)u * kTileRows);
        }
        if (any == 0) break;  // wave-uniform: nothing left in the iteration
#pragma unroll
        for (int u = 0; u < U; u++) {
            w[u][0] = live[u] & 1u ? star_word(tm, (uint32_t)v[u].x - tm.klo) : 0u;
            w[u][1] = live[u] & 2u ? star_word(tm, (uint32_t)v[u].y - tm.klo) : 0u;
            w[u][2] = live[u] & 4u ? star_word(tm, (uint32_t)v[u].z - tm.klo) : 0u;
            w[u][3] = live[u] & 8u ? star_word(tm, (uint32_t)v[u].w - tm.klo) : 0u;
        }
#pragma unroll
        for (int u = 0; u < U; u++)
            live[u] &= ((w[u][0] >> (((uint32_t)v[u].x - tm.klo) & 31u)) & 1u) | (((w[u][1] >> (((uint32_t)v[u].y - tm.klo) & 31u)) & 1u) << 1) |
                       (((w[u][2] >> (((uint32_t)v[u].z - tm.klo) & 31u)) & 1u) << 2) |
                       (((w[u][3] >> (((uint32_t)v[u].w - tm.klo) & 31u)) & 1u) << 3);
    }
}

// The ragged tile, row by row.
__device__ __forceinline__ uint32_t star_ragged(const WhereArgs& a, const StarArgs& s, uint64_t row, uint64_t end) {
    uint32_t live = live_ragged(a, row, end);
#pragma unroll
    for (int e = 0; e < 4; e++) {
        if (!(live & (1u << e))) continue;
        for (int j = 0; j < s.nterms; j++) {
            const uint32_t d = (uint32_t)s.t[j].col[row + e] - s.t[j].klo;
            if (!((star_word(s.t[j], d) >> (d & 31u)) & 1u)) {
                live &= ~(1u << e);
                break;
            }
        }
    }
    return live;
}

// k_where_mask's ballot words and counts, with the terms behind the ranges.
template <bool VEC>
__global__ __launch_bounds__(kTPB, 4) void k_star_mask(WhereArgs a, StarArgs s, uint64_t n, uint64_t rows_per_block,
                                                       u64* __restrict__ bm, uint32_t* __restrict__ cnt) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;

    auto put = [&](uint64_t t, uint32_t live) {
        const u64 w0 = __ballot(live & 1u), w1 = __ballot(live & 2u), w2 = __ballot(live & 4u), w3 = __ballot(live & 8u);
        const uint64_t wt = t / kWaveRows + (uint64_t)wave;
        if (lane < 4) bm[wt * 4 + lane] = lane == 0 ? w0 : lane == 1 ? w1 : lane == 2 ? w2 : w3;
        if (lane == 0) cnt[wt] = (uint32_t)(__popcll(w0) + __popcll(w1) + __popcll(w2) + __popcll(w3));
    };

    uint64_t t = start;
    for (; t + (uint64_t)kWhU * kTileRows <= end; t += (uint64_t)kWhU * kTileRows) {
        uint32_t live[kWhU];
        star_tiles<VEC, kWhU>(a, s, t + (uint64_t)tid * 4, lane, live);
#pragma unroll
        for (int u = 0; u < kWhU; u++) put(t + (uint64_t)u * kTileRows, live[u]);
    }
    for (; t + kTileRows <= end; t += kTileRows) {
        uint32_t live[1];
        star_tiles<VEC, 1>(a, s, t + (uint64_t)tid * 4, lane, live);
        put(t, live[0]);
    }
    if (t < end) put(t, star_ragged(a, s, t + (uint64_t)tid * 4, end));  // block-uniform
}

// The aggregate over no rows, in the stream's order.
__global__ void k_where_empty(mq_agg* __restrict__ out) {
    if (threadIdx.x || blockIdx.x) return;
    out->count = 0;
    out->sum = 0;
    out->min = INT32_MAX;
    out->max = INT32_MIN;
    out->_pad = 0;
}

// Where the pieces lie in the workspace, from n alone.
struct Layout {
    uint64_t nwt;  // wave tiles: whole 1024-row tiles (>= one)
    size_t bm, cnt, scan, total;
};

Layout layout(uint64_t n) {
    Layout l;
    const uint64_t tiles = n ? (n + kTileRows - 1) / kTileRows : 1;
    l.nwt = tiles * kWaves;
    l.bm = partial_bytes();
    l.cnt = l.bm + l.nwt * 4 * sizeof(u64);
    l.scan = l.cnt + (((l.nwt + 1) * sizeof(uint32_t) + 15) & ~(size_t)15);
    l.total = l.scan + scan_u32_scratch_elems(l.nwt + 1) * sizeof(u64);
    return l;
}

// What both entry points check and fold. `extra`: the payload (may be NULL) or the value
// column (must not be). Returns MQ_OK with *empty set when some range matches no int32;
// *vec: every column that is read lies on a 16-byte boundary.
// min_cols: 1, or 0 where a key predicate stands behind the ranges (d_cols and h_ranges may then be NULL).
int prepare(const char* who, int min_cols, const int32_t* const* d_cols, const mq_range* h_ranges, int ncols,
            const int32_t* extra, bool extra_needed, uint64_t n, const void* d_ws, size_t ws_bytes, WhereArgs* a, bool* empty,
            bool* vec) {
    if (ncols < min_cols || ncols > MQ_WHERE_MAX_COLS)
        return set_err(MQ_EINVAL, "%s: ncols %d outside %d..%d", who, ncols, min_cols, (int)MQ_WHERE_MAX_COLS);
    if (n >= (1ull << 31)) return set_err(MQ_EINVAL, "%s: n >= 2^31 (row ids are int32)", who);
    if (ncols && (!d_cols || !h_ranges)) return set_err(MQ_EINVAL, "%s: NULL columns or ranges", who);
    if (n) {
        for (int c = 0; c < ncols; c++)
            if (!d_cols[c] || (reinterpret_cast<uintptr_t>(d_cols[c]) & 3u))
                return set_err(MQ_EINVAL, "%s: column %d NULL or not 4-byte aligned", who, c);
        if ((extra_needed && !extra) || (reinterpret_cast<uintptr_t>(extra) & 3u))
            return set_err(MQ_EINVAL, "%s: %s NULL or not 4-byte aligned", who, extra_needed ? "value column" : "payload");
    }
    if (!d_ws || ws_bytes < layout(n).total || (reinterpret_cast<uintptr_t>(d_ws) & 15u))
        return set_err(MQ_EINVAL, "%s: workspace NULL, short or not 16-byte aligned", who);
    fold_ranges(d_cols, h_ranges, ncols, a, empty, vec);
    return MQ_OK;
}

// Dynamic LDS beyond 64 KiB has to be asked for, per kernel.
int allow_lds(const void* fn, size_t bytes) {
    if (bytes <= 48u * 1024u) return MQ_OK;
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return MQ_OK;
}

// The positions of the rows that `a` (and the key predicate `k`, when given) leave: the mask
// kernel, the scan and the expansion, on a checked workspace. lds: k's bitmap goes to LDS.
// star (without k): the filtering terms of mq_star_positions behind the ranges.
int run_positions(DevState* s, const WhereArgs& a, bool vec, const SemiArgs* k, bool lds, const int32_t* d_payload, uint64_t n,
                  int32_t* d_pos_out, uint64_t* d_count, void* d_ws, hipStream_t st, const StarArgs* star = nullptr) {
    const Layout l = layout(n);
    char* ws = static_cast<char*>(d_ws);
    u64* bm = reinterpret_cast<u64*>(ws + l.bm);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(ws + l.cnt);
    u64* scratch = reinterpret_cast<u64*>(ws + l.scan);
    uint32_t g;
    uint64_t rpb;
    int rc;
    HIPCHK(hipMemsetAsync(cnt + l.nwt, 0, sizeof(uint32_t), st));  // the scan's last input (its output is K)
    if (star) {
        geometry(s, n, vec ? reinterpret_cast<const void*>(&k_star_mask<true>) : reinterpret_cast<const void*>(&k_star_mask<false>),
                 &g, &rpb, (uint64_t)kWhU * kTileRows);
        if (vec)
            hipLaunchKernelGGL((k_star_mask<true>), dim3(g), dim3(kTPB), 0, st, a, *star, n, rpb, bm, cnt);
        else
            hipLaunchKernelGGL((k_star_mask<false>), dim3(g), dim3(kTPB), 0, st, a, *star, n, rpb, bm, cnt);
        LAUNCHCHK("k_star_mask");
    } else if (!k) {
        geometry(s, n, vec ? reinterpret_cast<const void*>(&k_where_mask<true>) : reinterpret_cast<const void*>(&k_where_mask<false>),
                 &g, &rpb, (uint64_t)kWhU * kTileRows);
        if (vec)
            hipLaunchKernelGGL((k_where_mask<true>), dim3(g), dim3(kTPB), 0, st, a, n, rpb, bm, cnt);
        else
            hipLaunchKernelGGL((k_where_mask<false>), dim3(g), dim3(kTPB), 0, st, a, n, rpb, bm, cnt);
        LAUNCHCHK("k_where_mask");
    } else {
        const size_t dyn = lds ? (size_t)k->vec16 * 16 : 0;
        const void* fn = vec ? (lds ? reinterpret_cast<const void*>(&k_semi_mask<true, true>) : reinterpret_cast<const void*>(&k_semi_mask<true, false>))
                             : (lds ? reinterpret_cast<const void*>(&k_semi_mask<false, true>) : reinterpret_cast<const void*>(&k_semi_mask<false, false>));
        if ((rc = allow_lds(fn, dyn))) return rc;
        geometry(s, n, fn, &g, &rpb, (uint64_t)kWhU * kTileRows, dyn);
        if (vec && lds)
            hipLaunchKernelGGL((k_semi_mask<true, true>), dim3(g), dim3(kTPB), dyn, st, a, *k, n, rpb, bm, cnt);
        else if (vec)
            hipLaunchKernelGGL((k_semi_mask<true, false>), dim3(g), dim3(kTPB), 0, st, a, *k, n, rpb, bm, cnt);
        else if (lds)
            hipLaunchKernelGGL((k_semi_mask<false, true>), dim3(g), dim3(kTPB), dyn, st, a, *k, n, rpb, bm, cnt);
        else
            hipLaunchKernelGGL((k_semi_mask<false, false>), dim3(g), dim3(kTPB), 0, st, a, *k, n, rpb, bm, cnt);
        LAUNCHCHK("k_semi_mask");
    }
    if ((rc = scan_u32_exclusive_u32(cnt, cnt, l.nwt + 1, scratch, st))) return rc;
    const uint32_t blocks = (uint32_t)((l.nwt + kExpWt - 1) / kExpWt);
    if (d_payload)
        hipLaunchKernelGGL((k_where_expand<true>), dim3(blocks), dim3(kTPB), 0, st, bm, cnt, (uint32_t)l.nwt, n, d_payload,
                           d_pos_out, reinterpret_cast<u64*>(d_count));
    else
        hipLaunchKernelGGL((k_where_expand<false>), dim3(blocks), dim3(kTPB), 0, st, bm, cnt, (uint32_t)l.nwt, n, d_payload,
                           d_pos_out, reinterpret_cast<u64*>(d_count));
    LAUNCHCHK("k_where_expand");
    return MQ_OK;
}

// The aggregate of d_val over those rows. vec: the predicate columns' alignment.
int run_agg(DevState* s, const WhereArgs& a, bool vec, const SemiArgs* k, bool lds, const int32_t* d_val, uint64_t n,
            mq_agg* d_out, void* d_ws, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    vec = vec && aligned16(d_val);
    uint32_t g;
    uint64_t rpb;
    Partial* part = static_cast<Partial*>(d_ws);
    if (!k) {
        geometry(s, n, vec ? reinterpret_cast<const void*>(&k_where_agg<true>) : reinterpret_cast<const void*>(&k_where_agg<false>),
                 &g, &rpb, (uint64_t)kWhU * kTileRows);
        if (vec)
            hipLaunchKernelGGL((k_where_agg<true>), dim3(g), dim3(kTPB), 0, st, a, d_val, n, rpb, part);
        else
            hipLaunchKernelGGL((k_where_agg<false>), dim3(g), dim3(kTPB), 0, st, a, d_val, n, rpb, part);
        LAUNCHCHK("k_where_agg");
    } else {
        const size_t dyn = lds ? (size_t)k->vec16 * 16 : 0;
        const void* fn = vec ? (lds ? reinterpret_cast<const void*>(&k_semi_agg<true, true>) : reinterpret_cast<const void*>(&k_semi_agg<true, false>))
                             : (lds ? reinterpret_cast<const void*>(&k_semi_agg<false, true>) : reinterpret_cast<const void*>(&k_semi_agg<false, false>));
        int rc;
        if ((rc = allow_lds(fn, dyn))) return rc;
        geometry(s, n, fn, &g, &rpb, (uint64_t)kWhU * kTileRows, dyn);
        if (vec && lds)
            hipLaunchKernelGGL((k_semi_agg<true, true>), dim3(g), dim3(kTPB), dyn, st, a, *k, d_val, n, rpb, part);
        else if (vec)
            hipLaunchKernelGGL((k_semi_agg<true, false>), dim3(g), dim3(kTPB), 0, st, a, *k, d_val, n, rpb, part);
        else if (lds)
            hipLaunchKernelGGL((k_semi_agg<false, true>), dim3(g), dim3(kTPB), dyn, st, a, *k, d_val, n, rpb, part);
        else
            hipLaunchKernelGGL((k_semi_agg<false, false>), dim3(g), dim3(kTPB), 0, st, a, *k, d_val, n, rpb, part);
        LAUNCHCHK("k_semi_agg");
    }
    return mq_combine_partials(d_ws, g, d_out, stream);
}

// AUTO copies the set into LDS up to kSemiLdsBytes; a forced LDS path takes what one block
// can hold beside the aggregate's partials (kSemiLdsMax).
// NOT YET MEASURED: 32 KiB keeps 5 blocks a CU resident (160 KiB of LDS); tools/bench_semi.py
// sweeps 2^14..2^17 bytes through both forced paths to settle it.
constexpr uint64_t kSemiLdsBytes = 32u * 1024u;
constexpr uint64_t kSemiLdsMax = 128u * 1024u;

// What mq_semi_positions and mq_semi_agg check and fold beyond prepare(). *lds: the path;
// *trivial: the set is empty (no key predicate is left: anti keeps every row, semi none).
int semi_prepare(const char* who, const int32_t* d_key, const mq_keyset* ks, int anti, int path, uint64_t n, bool* vec,
                 SemiArgs* k, bool* lds, bool* trivial) {
    if (!ks) return set_err(MQ_EINVAL, "%s: NULL key set", who);
    if (path != MQ_SEMI_AUTO && path != MQ_SEMI_LDS && path != MQ_SEMI_GLOBAL) return set_err(MQ_EINVAL, "%s: path %d", who, path);
    if (path == MQ_SEMI_LDS && ks->bytes > kSemiLdsMax)
        return set_err(MQ_EINVAL, "%s: a set of %llu bytes does not fit in LDS (%llu)", who, (u64)ks->bytes, (u64)kSemiLdsMax);
    if (n && (!d_key || (reinterpret_cast<uintptr_t>(d_key) & 3u))) return set_err(MQ_EINVAL, "%s: key column NULL or not 4-byte aligned", who);
    int dev = -1;
    int rc = current_device(&dev);
    if (rc) return rc;
    if (dev != ks->dev) return set_err(MQ_EINVAL, "%s: the key set lives on device %d, the call runs on %d", who, ks->dev, dev);
    *trivial = ks->lo > ks->hi;
    if (!*trivial) *vec = *vec && aligned16(d_key);  // an empty set: the key column is not read
    *k = SemiArgs{d_key, ks->bits, (uint32_t)ks->lo, (uint32_t)ks->hi - (uint32_t)ks->lo, (uint32_t)(ks->bytes / 16), anti ? 15u : 0u};
    *lds = path == MQ_SEMI_LDS || (path == MQ_SEMI_AUTO && ks->bytes <= kSemiLdsBytes);
    return MQ_OK;
}

}  // namespace

extern "C" {

size_t mq_where_workspace_bytes(uint64_t n) { return layout(n).total; }

int mq_where_positions(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols, const int32_t* d_payload,
                       uint64_t n, int32_t* d_pos_out, uint64_t* d_count, void* d_ws, size_t ws_bytes, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!d_count) return set_err(MQ_EINVAL, "mq_where_positions: NULL count");
    if (n && (!d_pos_out || (reinterpret_cast<uintptr_t>(d_pos_out) & 3u)))
        return set_err(MQ_EINVAL, "mq_where_positions: output NULL or not 4-byte aligned");
    WhereArgs a;
    bool empty, vec;
    if ((rc = prepare("mq_where_positions", 1, d_cols, h_ranges, ncols, d_payload, false, n, d_ws, ws_bytes, &a, &empty, &vec)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || empty) {
        HIPCHK(hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
        return MQ_OK;
    }
    return run_positions(s, a, vec, nullptr, false, d_payload, n, d_pos_out, d_count, d_ws, st);
}

int mq_where_agg(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols, const int32_t* d_val, uint64_t n,
                 mq_agg* d_out, void* d_ws, size_t ws_bytes, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!d_out) return set_err(MQ_EINVAL, "mq_where_agg: NULL output");
    WhereArgs a;
    bool empty, vec;
    if ((rc = prepare("mq_where_agg", 1, d_cols, h_ranges, ncols, d_val, true, n, d_ws, ws_bytes, &a, &empty, &vec))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || empty) {
        hipLaunchKernelGGL(k_where_empty, dim3(1), dim3(64), 0, st, d_out);
        LAUNCHCHK("k_where_empty");
        return MQ_OK;
    }
    return run_agg(s, a, vec, nullptr, false, d_val, n, d_out, d_ws, stream);
}

size_t mq_semi_workspace_bytes(uint64_t n) { return layout(n).total; }

int mq_semi_auto_path(uint64_t set_bytes) { return set_bytes <= kSemiLdsBytes ? MQ_SEMI_LDS : MQ_SEMI_GLOBAL; }

int mq_semi_positions(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols, const int32_t* d_key,
                      const mq_keyset* ks, int anti, int path, const int32_t* d_payload, uint64_t n, int32_t* d_pos_out,
                      uint64_t* d_count, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "mq_semi_positions";
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!d_count) return set_err(MQ_EINVAL, "%s: NULL count", who);
    if (n && (!d_pos_out || (reinterpret_cast<uintptr_t>(d_pos_out) & 3u)))
        return set_err(MQ_EINVAL, "%s: output NULL or not 4-byte aligned", who);
    WhereArgs a;
    SemiArgs k;
    bool empty, vec, lds, trivial;
    if ((rc = prepare(who, 0, d_cols, h_ranges, ncols, d_payload, false, n, d_ws, ws_bytes, &a, &empty, &vec))) return rc;
    if ((rc = semi_prepare(who, d_key, ks, anti, path, n, &vec, &k, &lds, &trivial))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || empty || (trivial && !anti)) {
        HIPCHK(hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
        return MQ_OK;
    }
    // NOT IN the empty set: the ranges alone, as mq_where_positions runs them
    if (trivial) return run_positions(s, a, vec, nullptr, false, d_payload, n, d_pos_out, d_count, d_ws, st);
    return run_positions(s, a, vec, &k, lds, d_payload, n, d_pos_out, d_count, d_ws, st);
}

int mq_star_positions(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols, const mq_star_term* h_terms, int nterms,
                      const int32_t* d_payload, uint64_t n, int32_t* d_pos_out, uint64_t* d_count, void* d_ws, size_t ws_bytes,
                      void* stream) {
    const char* who = "mq_star_positions";
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!d_count) return set_err(MQ_EINVAL, "%s: NULL count", who);
    if (nterms < 1 || nterms > MQ_STAR_MAX_TERMS) return set_err(MQ_EINVAL, "%s: nterms %d outside 1..%d", who, nterms, (int)MQ_STAR_MAX_TERMS);
    if (!h_terms) return set_err(MQ_EINVAL, "%s: NULL terms", who);
    if (n && (!d_pos_out || (reinterpret_cast<uintptr_t>(d_pos_out) & 3u)))
        return set_err(MQ_EINVAL, "%s: output NULL or not 4-byte aligned", who);
    WhereArgs a;
    bool empty, vec;
    if ((rc = prepare(who, 0, d_cols, h_ranges, ncols, d_payload, false, n, d_ws, ws_bytes, &a, &empty, &vec))) return rc;
    int dev = -1;
    if ((rc = current_device(&dev))) return rc;
    StarArgs sa = {};
    bool none = false;  // an empty map or set: no row is joined
    for (int j = 0; j < nterms; j++) {
        const mq_star_term& t = h_terms[j];
        if (t.km && t.ks) return set_err(MQ_EINVAL, "%s: term %d has both a key map and a key set", who, j);
        if (n && (!t.d_col || (reinterpret_cast<uintptr_t>(t.d_col) & 3u)))
            return set_err(MQ_EINVAL, "%s: term %d: column NULL or not 4-byte aligned", who, j);
        const mq_keyset* ks = t.km ? t.km->ks : t.ks;
        if (!ks) continue;  // a plain term places no condition
        if (dev != ks->dev) return set_err(MQ_EINVAL, "%s: term %d: the key %s lives on device %d, the call runs on %d", who, j,
                                           t.km ? "map" : "set", ks->dev, dev);
        if (ks->lo > ks->hi) {
            none = true;
            continue;
        }
        StarTerm& o = sa.t[sa.nterms++];
        o.col = t.d_col;
        o.bits = ks->bits;
        o.klo = (uint32_t)ks->lo;
        o.kwm1 = (uint32_t)ks->hi - (uint32_t)ks->lo;
        o.kind = kStarSet;
        vec = vec && aligned16(t.d_col);
    }
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || empty || none) {
        HIPCHK(hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
        return MQ_OK;
    }
    return run_positions(s, a, vec, nullptr, false, d_payload, n, d_pos_out, d_count, d_ws, st, &sa);
}

int mq_semi_agg(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols, const int32_t* d_key, const mq_keyset* ks,
                int anti, int path, const int32_t* d_val, uint64_t n, mq_agg* d_out, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "mq_semi_agg";
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!d_out) return set_err(MQ_EINVAL, "%s: NULL output", who);
    WhereArgs a;
    SemiArgs k;
    bool empty, vec, lds, trivial;
    if ((rc = prepare(who, 0, d_cols, h_ranges, ncols, d_val, true, n, d_ws, ws_bytes, &a, &empty, &vec))) return rc;
    if ((rc = semi_prepare(who, d_key, ks, anti, path, n, &vec, &k, &lds, &trivial))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || empty || (trivial && !anti)) {
        hipLaunchKernelGGL(k_where_empty, dim3(1), dim3(64), 0, st, d_out);
        LAUNCHCHK("k_where_empty");
        return MQ_OK;
    }
    // NOT IN the empty set: the ranges alone, as mq_where_agg runs them
    if (trivial) return run_agg(s, a, vec, nullptr, false, d_val, n, d_out, d_ws, stream);
    return run_agg(s, a, vec, &k, lds, d_val, n, d_out, d_ws, stream);
}

}  // extern "C"
