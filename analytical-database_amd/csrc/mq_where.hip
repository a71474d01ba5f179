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
int prepare(const char* who, const int32_t* const* d_cols, const mq_range* h_ranges, int ncols, const int32_t* extra,
            bool extra_needed, uint64_t n, const void* d_ws, size_t ws_bytes, WhereArgs* a, bool* empty, bool* vec) {
    if (ncols < 1 || ncols > MQ_WHERE_MAX_COLS) return set_err(MQ_EINVAL, "%s: ncols %d outside 1..%d", who, ncols, (int)MQ_WHERE_MAX_COLS);
    if (n >= (1ull << 31)) return set_err(MQ_EINVAL, "%s: n >= 2^31 (row ids are int32)", who);
    if (!d_cols || !h_ranges) return set_err(MQ_EINVAL, "%s: NULL columns or ranges", who);
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
    if ((rc = prepare("mq_where_positions", d_cols, h_ranges, ncols, d_payload, false, n, d_ws, ws_bytes, &a, &empty, &vec)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || empty) {
        HIPCHK(hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
        return MQ_OK;
    }
    const Layout l = layout(n);
    char* ws = static_cast<char*>(d_ws);
    u64* bm = reinterpret_cast<u64*>(ws + l.bm);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(ws + l.cnt);
    u64* scratch = reinterpret_cast<u64*>(ws + l.scan);
    uint32_t g;
    uint64_t rpb;
    geometry(s, n, vec ? reinterpret_cast<const void*>(&k_where_mask<true>) : reinterpret_cast<const void*>(&k_where_mask<false>),
             &g, &rpb, (uint64_t)kWhU * kTileRows);
    HIPCHK(hipMemsetAsync(cnt + l.nwt, 0, sizeof(uint32_t), st));  // the scan's last input (its output is K)
    if (vec)
        hipLaunchKernelGGL((k_where_mask<true>), dim3(g), dim3(kTPB), 0, st, a, n, rpb, bm, cnt);
    else
        hipLaunchKernelGGL((k_where_mask<false>), dim3(g), dim3(kTPB), 0, st, a, n, rpb, bm, cnt);
    LAUNCHCHK("k_where_mask");
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

int mq_where_agg(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols, const int32_t* d_val, uint64_t n,
                 mq_agg* d_out, void* d_ws, size_t ws_bytes, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!d_out) return set_err(MQ_EINVAL, "mq_where_agg: NULL output");
    WhereArgs a;
    bool empty, vec;
    if ((rc = prepare("mq_where_agg", d_cols, h_ranges, ncols, d_val, true, n, d_ws, ws_bytes, &a, &empty, &vec))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || empty) {
        hipLaunchKernelGGL(k_where_empty, dim3(1), dim3(64), 0, st, d_out);
        LAUNCHCHK("k_where_empty");
        return MQ_OK;
    }
    vec = vec && aligned16(d_val);
    uint32_t g;
    uint64_t rpb;
    geometry(s, n, vec ? reinterpret_cast<const void*>(&k_where_agg<true>) : reinterpret_cast<const void*>(&k_where_agg<false>),
             &g, &rpb, (uint64_t)kWhU * kTileRows);
    Partial* part = static_cast<Partial*>(d_ws);
    if (vec)
        hipLaunchKernelGGL((k_where_agg<true>), dim3(g), dim3(kTPB), 0, st, a, d_val, n, rpb, part);
    else
        hipLaunchKernelGGL((k_where_agg<false>), dim3(g), dim3(kTPB), 0, st, a, d_val, n, rpb, part);
    LAUNCHCHK("k_where_agg");
    return mq_combine_partials(d_ws, g, d_out, stream);
}

}  // extern "C"
