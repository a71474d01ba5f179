// mq_distinct.hip — COUNT(DISTINCT v) per group under a WHERE:
//   SELECT k0, .., count(DISTINCT v) FROM t WHERE c0 IN [..) AND .. GROUP BY k0, ..
// One entry per distinct key tuple with a matching row, in ascending lexicographic order
// (mq_group_by_where_plan's), each with the number of different values among its matching rows.
// Integer compares and bit sets only: the result does not depend on the path, the grid, the
// alignment, the order of the predicates or the order in which blocks finish.
//
// With P = the key space of the bounds, W = the value span and R = ceil(W / 32), a group's values
// are one row of R 32-bit words in a bitmap of P rows; the padding bits are never set.
//   lds    (4 P R <= mq_group_distinct_lds_bytes()):
//     k_gdistinct_mark<NK, VEC, true>: k_group_by_where_dense's stream (live_tiles / live_ragged,
//       then of the key and value columns the 128-byte lines that hold a survivor); a survivor
//       sets bit code * 32 R + (v - vlo) in the block's LDS bitmap (ds_or_b32); at the end of its
//       chunk the block ORs its non-zero words into the zeroed global bitmap.
//   bitmap (4 P R <= mq_group_distinct_bitmap_bytes()):
//     k_gdistinct_mark<NK, VEC, false>: the same stream marking the global bitmap directly with
//       k_keyset_build's load-then-atomicOr (a hot pair does not queue n atomics on one address).
//   both: k_gdistinct_rows writes popcount(row) per code (a thread a row for short rows, a wave
//       per 4096-word piece of a row otherwise, pieces of one row added up atomically);
//       mq_select_positions with low = 1 over those counts gives the non-empty codes in order,
//       mq_fetch their counts.
//   sort   (P <= 2^32, any W): mq_where_positions; k_group_by_pack(_pos) the codes; mq_fetch the
//     values; mq_index_build by value, mq_gather_u64 the codes into value order, mq_index_build by
//     code (stable, so the rows are in (code, value) order), mq_gather_u64 the values along;
//     k_gdistinct_heads counts a chunk's group heads and pair heads (a row whose code or value
//     differs from the row before it), k_gdistinct_seg_write adds up the pair heads of every run.
// The handle keeps the groups' codes and counts only; the write decodes the codes
// (k_group_by_unpack) and widens the counts.

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <new>
#include <type_traits>

#include "mq_common.h"
#include "mq_device.h"
#include "mq_group_impl.h"
#include "mq_scan_common.h"
#include "mq_where_common.h"

struct mq_gdistinct {
    int dev;
    int nkeys;
    uint64_t groups;
    hipStream_t stream;  // of the last call that queued work on the buffers below
    int32_t* codes;      // [groups] ascending tuple codes
    int32_t* counts;     // [groups] distinct values, each at most n < 2^31
    // the tuple behind a code: K_j = klo[j] + (code / kstride[j]) % (krm1[j] + 1)
    int32_t klo[MQ_GROUP_MAX_KEYS];
    uint32_t krm1[MQ_GROUP_MAX_KEYS];
    uint32_t kstride[MQ_GROUP_MAX_KEYS];
};

namespace {

using namespace mqi;
using u64 = unsigned long long;

constexpr int kMaxKeys = MQ_GROUP_MAX_KEYS;
// NOT SWEPT: the LDS table size of every dense grouping kernel of the library (4 blocks a CU).
constexpr uint64_t kLdsBytes = 40960;
constexpr uint32_t kLdsWords = kLdsBytes / 4;
constexpr uint64_t kBitmapBytes = 512ull << 20;  // the key set's bitmap at the full int32 span
constexpr uint32_t kRowThread = 16;              // rows of up to this many words: a thread a row
constexpr uint32_t kPiece = 4096;                // words of a longer row that one wave counts
constexpr int kSegU = 4;
constexpr int kSegTile = kTPB * kSegU;

// Tiles of each column in flight per thread: (nkeys + 1) * U dwordx4 of loaded data a lane, as
// k_group_by_where_dense keeps them. NOT SWEPT.
constexpr int mark_tiles(int nkeys) { return nkeys <= 2 ? 4 : nkeys == 3 ? 3 : 2; }

// The stream of k_group_by_where_dense with the value's bit in place of the table update. A
// matching row with a key component or the value out of bounds is counted and never used as an
// address; a row that fails a predicate is never looked at. cnt[0][block][wave] = those rows,
// cnt[1][block][wave] = the matching rows. words = P * R <= 2^27, and <= kLdsWords with LDS.
template <int NK, bool VEC, bool LDS>
__global__ __launch_bounds__(kTPB, 4) void k_gdistinct_mark(WhereArgs w, ByArgs a, const int* vals, uint32_t vlo, uint32_t vwm1,
                                                            uint32_t R, uint32_t words, uint64_t n, uint64_t rows_per_block,
                                                            uint32_t* __restrict__ bits, uint32_t* __restrict__ cnt) {
    constexpr int U = mark_tiles(NK);
    __shared__ uint32_t s_bits[LDS ? kLdsWords : 1];
    const int tid = threadIdx.x, lane = tid & 63;
    if constexpr (LDS) {
        for (uint32_t q = tid; q < words; q += kTPB) s_bits[q] = 0u;
        __syncthreads();
    }
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;

    uint32_t nbad = 0, nrows = 0;
    auto mark = [&](bool ok, uint32_t code, int v) {
        const uint32_t d = (uint32_t)v - vlo;
        if (!ok || d > vwm1) {
            nbad++;
            return;
        }
        const uint32_t idx = code * R + (d >> 5);  // <= (P - 1) R + R - 1 < words
        const uint32_t m = 1u << (d & 31u);
        if constexpr (LDS) {
            atomicOr(&s_bits[idx], m);
        } else {
            uint32_t* p = bits + idx;
            if (!(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m)) atomicOr(p, m);
        }
    };
    auto consume = [&](const int4 (&k)[NK], int4 v, uint32_t live) {
        uint32_t in;
        const uint4 c = tile_codes<NK>(a, k, &in);  // of a dead row: never read below
        nrows += (uint32_t)__popc(live);
        if (live & 1u) mark(in & 1u, c.x, v.x);
        if (live & 2u) mark(in & 2u, c.y, v.y);
        if (live & 4u) mark(in & 4u, c.z, v.z);
        if (live & 8u) mark(in & 8u, c.w, v.w);
    };
    // T full tiles: every key and value load of the iteration is issued before the first use
    auto tiles = [&](auto tc, uint64_t t) {
        constexpr int T = decltype(tc)::value;
        const uint64_t row = t + (uint64_t)tid * 4;
        uint32_t live[T];
        live_tiles<VEC, T>(w, row, lane, live);
        u64 b[T];
        int4 k[T][NK], v[T];
#pragma unroll
        for (int u = 0; u < T; u++) {
            b[u] = __ballot(live[u] != 0u);
            v[u] = make_int4(0, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NK; j++) k[u][j] = make_int4(0, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < NK; j++)
#pragma unroll
            for (int u = 0; u < T; u++)
                if (b[u] != 0 && line_live(b[u], lane)) k[u][j] = load4_nt<VEC>(a.keys[j] + row + (uint64_t)u * kTileRows);
#pragma unroll
        for (int u = 0; u < T; u++)
            if (b[u] != 0 && line_live(b[u], lane)) v[u] = load4_nt<VEC>(vals + row + (uint64_t)u * kTileRows);
#pragma unroll
        for (int u = 0; u < T; u++)
            if (live[u] != 0u) consume(k[u], v[u], live[u]);
    };

    uint64_t t = start;
    for (; t + (uint64_t)U * kTileRows <= end; t += (uint64_t)U * kTileRows) tiles(std::integral_constant<int, U>{}, t);
    for (; t + kTileRows <= end; t += kTileRows) tiles(std::integral_constant<int, 1>{}, t);
    if (t < end) {  // the column's ragged tile: row by row, none past the end
        const uint64_t row = t + (uint64_t)tid * 4;
        const uint32_t live = live_ragged(w, row, end);
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (live & (1u << e)) {
                int r[NK];
#pragma unroll
                for (int j = 0; j < NK; j++) r[j] = a.keys[j][row + e];
                bool ok;
                const uint32_t c = row_code<NK>(a, r, &ok);
                nrows++;
                mark(ok, c, vals[row + e]);
            }
    }
    nbad = (uint32_t)wave_sum_u64(nbad);
    nrows = (uint32_t)wave_sum_u64(nrows);  // <= the rows of the block's chunk < 2^31
    if (lane == 0) {
        const size_t slot = (size_t)blockIdx.x * kWaves + (tid >> 6);
        cnt[slot] = nbad;
        cnt[(size_t)gridDim.x * kWaves + slot] = nrows;
    }
    if constexpr (LDS) {
        __syncthreads();
        for (uint32_t q = tid; q < words; q += kTPB) {
            const uint32_t x = s_bits[q];
            if (x) atomicOr(bits + q, x);
        }
    }
}

// counts[code] = popcount of the code's R words, rows of up to kRowThread words: a thread a row
// (grid-stride over the P rows).
__global__ __launch_bounds__(kTPB) void k_gdistinct_rows_short(const uint32_t* __restrict__ bits, uint32_t P, uint32_t R,
                                                               int32_t* __restrict__ counts) {
    for (u64 c = (u64)blockIdx.x * kTPB + threadIdx.x; c < P; c += (u64)gridDim.x * kTPB) {
        const uint32_t* __restrict__ p = bits + c * R;
        uint32_t s = 0;
        for (uint32_t q = 0; q < R; q++) s += (uint32_t)__popc(p[q]);
        counts[c] = (int32_t)s;
    }
}

// Longer rows: a wave per piece of kPiece words (pieces = ceil(R / kPiece) a row, grid-stride over
// the P * pieces units); a row of one piece is stored, the pieces of a longer row are added onto
// the zeroed count.
__global__ __launch_bounds__(kTPB) void k_gdistinct_rows_long(const uint32_t* __restrict__ bits, uint32_t P, uint32_t R,
                                                              uint32_t pieces, int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const u64 units = (u64)P * pieces;
    for (u64 unit = (u64)blockIdx.x * kWaves + (threadIdx.x >> 6); unit < units; unit += (u64)gridDim.x * kWaves) {
        const uint32_t c = (uint32_t)(unit / pieces), piece = (uint32_t)(unit % pieces);
        const uint32_t q0 = piece * kPiece;
        const uint32_t q1 = R - q0 < kPiece ? R : q0 + kPiece;
        const uint32_t* __restrict__ p = bits + (u64)c * R;
        uint32_t s = 0;
        for (uint32_t q = q0 + lane; q < q1; q += 64) s += (uint32_t)__popc(p[q]);
        s = (uint32_t)wave_sum_u64(s);
        if (lane == 0) {
            if (pieces == 1) counts[c] = (int32_t)s;
            else if (s) atomicAdd(counts + c, (int32_t)s);
        }
    }
}

// out[i] = counts[i] as u64, i < groups.
__global__ __launch_bounds__(kTPB) void k_gdistinct_widen(const int32_t* __restrict__ counts, u64 groups, u64* __restrict__ out) {
    for (u64 i = (u64)blockIdx.x * kTPB + threadIdx.x; i < groups; i += (u64)gridDim.x * kTPB) out[i] = (u64)(uint32_t)counts[i];
}

// ---- the sort path: rows in (code, value) order ----

// ccnt[b] = group heads (the code differs from the row before) in block b's chunk; tot[0] += them,
// tot[1] += the pair heads (the code or the value differs).
__global__ __launch_bounds__(kTPB) void k_gdistinct_heads(const int32_t* __restrict__ codes, const int32_t* __restrict__ vals,
                                                          uint32_t n, uint64_t chunk, uint32_t* __restrict__ ccnt,
                                                          u64* __restrict__ tot) {
    __shared__ uint32_t s_w[kWaves];
    const uint64_t i0 = (uint64_t)blockIdx.x * chunk;
    const uint64_t i1 = i0 + chunk < n ? i0 + chunk : n;
    uint32_t h = 0, ph = 0;
    for (uint64_t i = i0 + threadIdx.x; i < i1; i += kTPB) {
        const bool head = i == 0 || codes[i] != codes[i - 1];
        h += head;
        ph += head || vals[i] != vals[i - 1];
    }
    const uint32_t heads = block_sum(h, s_w);
    const uint32_t pairs = block_sum(ph, s_w);
    if (threadIdx.x == 0) {
        ccnt[blockIdx.x] = heads;
        if (heads) atomicAdd(tot, (u64)heads);
        if (pairs) atomicAdd(tot + 1, (u64)pairs);
    }
}

// Row i belongs to group (group heads in [0, i]) - 1. Within a tile of kSegTile rows, local slot
// l = the tile's group heads up to and including the row: slot 0 continues the run open before
// the tile, slot nh is open at its end, the slots between begin and end inside the tile. A
// slot's pair heads are counted in LDS; the slots between are stored, slot 0 and slot nh, which
// other tiles and chunks may share, are added onto the zeroed counts. codes_out[g] = the group's
// code, unflipped.
__global__ __launch_bounds__(kTPB) void k_gdistinct_seg_write(const int32_t* __restrict__ codes, const int32_t* __restrict__ vals,
                                                              uint32_t n, uint64_t chunk, const uint32_t* __restrict__ ccnt,
                                                              u64 groups, int32_t* __restrict__ codes_out,
                                                              int32_t* __restrict__ counts) {
    __shared__ uint32_t s_c[kSegTile + 1];
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint32_t s_hc[kSegU][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t below = 0;
    for (uint32_t i = tid; i < blockIdx.x; i += kTPB) below += ccnt[i];
    u64 base = block_sum(below, s_w);  // group heads before the tile (< 2^31)
    const uint64_t i0 = (uint64_t)blockIdx.x * chunk;
    const uint64_t i1 = i0 + chunk < n ? i0 + chunk : n;
    for (uint64_t s = i0; s < i1; s += kSegTile) {  // block-uniform trip count
        for (uint32_t q = tid; q <= (uint32_t)kSegTile; q += kTPB) s_c[q] = 0u;
        int32_t k[kSegU];
        bool ok[kSegU], h[kSegU], ph[kSegU];
        uint32_t in_wave[kSegU];
#pragma unroll
        for (int u = 0; u < kSegU; u++) {
            const uint64_t i = s + (uint64_t)u * kTPB + tid;
            ok[u] = i < i1;
            k[u] = ok[u] ? codes[i] : 0;
            h[u] = ok[u] && (i == 0 || k[u] != codes[i - 1]);
            ph[u] = h[u] || (ok[u] && vals[i] != vals[i - 1]);
            const u64 m = __ballot(h[u]);
            in_wave[u] = lanes_below(m);
            if (lane == 0) s_hc[u][wave] = (uint32_t)__popcll(m);
        }
        __syncthreads();  // the slots are zero, the head counts are in
        uint32_t nh = 0;
#pragma unroll
        for (int u = 0; u < kSegU; u++) {
            uint32_t mine = nh;
#pragma unroll
            for (int w = 0; w < kWaves; w++) {
                const uint32_t c = s_hc[u][w];
                mine += w < wave ? c : 0u;
                nh += c;
            }
            if (!ok[u]) continue;
            const uint32_t l = mine + in_wave[u] + (h[u] ? 1u : 0u);  // <= rows before + 1 <= kSegTile
            if (ph[u]) atomicAdd(&s_c[l], 1u);
            if (h[u] && base + l - 1 < groups) codes_out[base + l - 1] = (int32_t)((uint32_t)k[u] ^ 0x80000000u);
        }
        __syncthreads();
        for (uint32_t q = tid; q <= nh; q += kTPB) {
            const uint32_t c = s_c[q];
            if (base + q == 0 || base + q - 1 >= groups) continue;  // never: row 0 is a head, the plan counted the same heads
            int32_t* o = counts + (base + q - 1);
            if (q == 0 || q == nh) {
                if (c) atomicAdd(o, (int32_t)c);
            } else {
                *o = (int32_t)c;
            }
        }
        base += nh;
        __syncthreads();  // the slots and head counts are read before the next tile resets them
    }
}

// ---- host ----

struct Shape {
    uint64_t space;  // P, saturated at 2^63
    uint64_t span;   // W
    uint64_t rwords; // R
    uint64_t bytes;  // 4 P R, ~0 when P > 2^32
};

// false: a lo > hi among the bounds.
bool shape_of(const int32_t* kb, int nkeys, const int32_t* vb, Shape* sh) {
    if (!group_key_space(kb, nkeys, &sh->space) || vb[0] > vb[1]) return false;
    sh->span = (uint64_t)((int64_t)vb[1] - (int64_t)vb[0] + 1);
    sh->rwords = (sh->span + 31) / 32;
    sh->bytes = sh->space > (1ull << 32) ? ~0ull : 4 * sh->space * sh->rwords;  // <= 2^61
    return true;
}

int auto_of(const Shape& sh) {
    return sh.bytes <= kLdsBytes ? MQ_GDISTINCT_LDS : sh.bytes <= kBitmapBytes ? MQ_GDISTINCT_BITMAP : MQ_GDISTINCT_SORT;
}

void release(mq_gdistinct* g, hipStream_t st) {
    pool_free_on(g->codes, st);
    pool_free_on(g->counts, st);
    delete g;
}

template <int NK, bool VEC, bool LDS>
int launch_mark(const DevState* s, const WhereArgs& w, const ByArgs& a, const int32_t* vals, uint32_t vlo, uint32_t vwm1, uint32_t R,
                uint32_t words, uint64_t n, uint32_t* bits, uint32_t** cnt_out, uint32_t* ncnt_out, hipStream_t st) {
    uint32_t g;
    uint64_t rpb;
    geometry(s, n, reinterpret_cast<const void*>(&k_gdistinct_mark<NK, VEC, LDS>), &g, &rpb, (uint64_t)mark_tiles(NK) * kTileRows);
    uint32_t* cnt = static_cast<uint32_t*>(pool_alloc((size_t)2 * g * kWaves * 4));
    if (!cnt) return set_err(MQ_ENOMEM, "mq_group_distinct_plan: allocation failed");
    *cnt_out = cnt;
    *ncnt_out = g * kWaves;
    hipLaunchKernelGGL((k_gdistinct_mark<NK, VEC, LDS>), dim3(g), dim3(kTPB), 0, st, w, a, vals, vlo, vwm1, R, words, n, rpb, bits, cnt);
    LAUNCHCHK("k_gdistinct_mark");
    return MQ_OK;
}

// The two bitmap paths: mark, count the rows' bits, compact the non-empty rows. Synchronises.
int plan_bitmap(const DevState* s, mq_gdistinct* g, bool lds, const WhereArgs& w, bool vec, const ByArgs& a, const int32_t* d_vals,
                int32_t vlo, const Shape& sh, uint64_t n, uint64_t* rows, uint64_t* pairs, hipStream_t st) {
    const char* who = "mq_group_distinct_plan";
    const uint32_t P = (uint32_t)sh.space, R = (uint32_t)sh.rwords;  // P R <= 2^27
    const uint32_t words = P * R;
    const uint32_t vwm1 = (uint32_t)(sh.span - 1);
    const size_t ws_bytes = mq_scan_workspace_bytes(P);
    uint32_t* bits = static_cast<uint32_t*>(pool_alloc((size_t)words * 4));
    int32_t* counts = static_cast<int32_t*>(pool_alloc((size_t)P * 4));
    int32_t* pos = static_cast<int32_t*>(pool_alloc((size_t)P * 4));
    void* ws = pool_alloc(ws_bytes);
    char* small = static_cast<char*>(pool_alloc(4 * sizeof(u64) + sizeof(mq_agg)));  // {bad, rows, k, pad}, the counts' aggregate
    uint32_t* cnt = nullptr;
    uint32_t ncnt = 0;
    u64* d_tot = reinterpret_cast<u64*>(small);
    mq_agg* d_agg = reinterpret_cast<mq_agg*>(small + 4 * sizeof(u64));
    auto done = [&](int code) {
        pool_free_on(bits, st);
        pool_free_on(counts, st);
        pool_free_on(pos, st);
        pool_free_on(ws, st);
        pool_free_on(small, st);
        pool_free_on(cnt, st);
        return code;
    };
    if (!bits || !counts || !pos || !ws || !small) return done(set_err(MQ_ENOMEM, "%s: allocation failed (%llu bytes of bitmap)", who, (u64)sh.bytes));
    if (hipMemsetAsync(bits, 0, (size_t)words * 4, st) != hipSuccess) return done(set_err(MQ_EHIP, "%s: memset failed", who));
    auto with_nk = [&](auto nk) {
        constexpr int NK = decltype(nk)::value;
        const uint32_t lo = (uint32_t)vlo;
        if (lds)
            return vec ? launch_mark<NK, true, true>(s, w, a, d_vals, lo, vwm1, R, words, n, bits, &cnt, &ncnt, st)
                       : launch_mark<NK, false, true>(s, w, a, d_vals, lo, vwm1, R, words, n, bits, &cnt, &ncnt, st);
        return vec ? launch_mark<NK, true, false>(s, w, a, d_vals, lo, vwm1, R, words, n, bits, &cnt, &ncnt, st)
                   : launch_mark<NK, false, false>(s, w, a, d_vals, lo, vwm1, R, words, n, bits, &cnt, &ncnt, st);
    };
    int rc = g->nkeys == 1   ? with_nk(std::integral_constant<int, 1>{})
             : g->nkeys == 2 ? with_nk(std::integral_constant<int, 2>{})
             : g->nkeys == 3 ? with_nk(std::integral_constant<int, 3>{})
                             : with_nk(std::integral_constant<int, 4>{});
    if (rc) return done(rc);
    group_launch_bad_total(cnt, ncnt, d_tot, st);
    group_launch_bad_total(cnt + ncnt, ncnt, d_tot + 1, st);
    if (R <= kRowThread) {
        hipLaunchKernelGGL(k_gdistinct_rows_short, dim3(stream_grid(s, P)), dim3(kTPB), 0, st, bits, P, R, counts);
    } else {
        const uint32_t pieces = (R + kPiece - 1) / kPiece;
        if (pieces > 1 && hipMemsetAsync(counts, 0, (size_t)P * 4, st) != hipSuccess) return done(set_err(MQ_EHIP, "%s: memset failed", who));
        hipLaunchKernelGGL(k_gdistinct_rows_long, dim3(stream_grid(s, (uint64_t)P * pieces * 64)), dim3(kTPB), 0, st, bits, P, R, pieces,
                           counts);
    }
    if (hipGetLastError() != hipSuccess) return done(set_err(MQ_EHIP, "%s: launch of the count kernels failed", who));
    rc = mq_select_positions(counts, nullptr, P, 1, 1, 0, 0, pos, reinterpret_cast<uint64_t*>(d_tot + 2), ws, ws_bytes, st);
    if (rc) return done(rc);
    u64 h[3] = {0, 0, 0};
    if (hipMemcpyAsync(h, d_tot, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return done(set_err(MQ_EHIP, "%s: header download failed", who));
    if (h[0]) return done(set_err(MQ_EINVAL, "%s: %llu matching rows with a key or the value outside its bounds", who, h[0]));
    *rows = h[1];
    const u64 k = h[2];
    if (k) {
        g->codes = static_cast<int32_t*>(pool_alloc(k * 4));
        g->counts = static_cast<int32_t*>(pool_alloc(k * 4));
        if (!g->codes || !g->counts) return done(set_err(MQ_ENOMEM, "%s: allocation failed", who));
        if (hipMemcpyAsync(g->codes, pos, k * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
            return done(set_err(MQ_EHIP, "%s: copy of the codes failed", who));
        if ((rc = mq_fetch(counts, pos, k, g->counts, st))) return done(rc);
        if ((rc = mq_reduce(g->counts, k, d_agg, ws, ws_bytes, st))) return done(rc);
        mq_agg ag = {};
        if (hipMemcpyAsync(&ag, d_agg, sizeof ag, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return done(set_err(MQ_EHIP, "%s: count download failed", who));
        *pairs = (uint64_t)ag.sum;
    }
    g->groups = k;
    return done(MQ_OK);
}

// The sort path. have_vb: value bounds were given, and the matching rows' values are checked
// against them (one mq_reduce). Synchronises.
int plan_sort(const DevState* s, mq_gdistinct* g, const int32_t* const* d_cols, const mq_range* h_ranges, int ncols, const ByArgs& a,
              const int32_t* d_vals, bool have_vb, const int32_t* vb, uint64_t n, uint64_t* rows, uint64_t* pairs, hipStream_t st) {
    const char* who = "mq_group_distinct_plan";
    void* stream = (void*)st;
    int32_t *pos = nullptr, *packed = nullptr, *v = nullptr, *va = nullptr, *ca = nullptr, *cs = nullptr, *vf = nullptr;
    uint64_t *pa = nullptr, *pb = nullptr;
    void* ws = nullptr;
    char* small = nullptr;
    uint32_t *bad = nullptr, *ccnt = nullptr;
    auto done = [&](int code) {
        for (void* p : {(void*)pos, (void*)packed, (void*)v, (void*)va, (void*)ca, (void*)cs, (void*)vf, (void*)pa, (void*)pb, ws,
                        (void*)small, (void*)bad, (void*)ccnt})
            pool_free_on(p, st);
        return code;
    };
    auto oom = [&]() { return done(set_err(MQ_ENOMEM, "%s: allocation failed", who)); };
    const size_t ws_bytes = ncols ? mq_where_workspace_bytes(n) : mq_scan_workspace_bytes(0);
    small = static_cast<char*>(pool_alloc(4 * sizeof(u64) + sizeof(mq_agg)));  // {k, bad, heads, pair heads}, the values' aggregate
    ws = pool_alloc(ws_bytes);
    if (!small || !ws) return oom();
    u64* d_hdr = reinterpret_cast<u64*>(small);
    mq_agg* d_agg = reinterpret_cast<mq_agg*>(small + 4 * sizeof(u64));
    int rc;
    u64 k = n;
    if (ncols) {
        if (!(pos = static_cast<int32_t*>(pool_alloc(n * 4)))) return oom();
        if ((rc = mq_where_positions(d_cols, h_ranges, ncols, nullptr, n, pos, reinterpret_cast<uint64_t*>(d_hdr), ws, ws_bytes, stream)))
            return done(rc);
        if (hipMemcpyAsync(&k, d_hdr, sizeof k, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return done(set_err(MQ_EHIP, "%s: count download failed", who));
    }
    *rows = k;
    if (k == 0) return done(MQ_OK);
    uint32_t nbad = 0;
    if (!(packed = static_cast<int32_t*>(pool_alloc(k * 4)))) return oom();
    if ((rc = group_launch_pack(s, a, g->nkeys, n, pos, k, packed, &bad, &nbad, st))) return done(rc);
    group_launch_bad_total(bad, nbad, d_hdr + 1, st);
    if (hipGetLastError() != hipSuccess) return done(set_err(MQ_EHIP, "%s: launch of k_group_by_bad failed", who));
    const int32_t* vals = d_vals;  // every row matches: the column itself
    if (pos) {
        if (!(v = static_cast<int32_t*>(pool_alloc(k * 4)))) return oom();
        if ((rc = mq_fetch(d_vals, pos, k, v, stream))) return done(rc);
        vals = v;
    }
    if (have_vb && (rc = mq_reduce(vals, k, d_agg, ws, ws_bytes, stream))) return done(rc);
    u64 h[2] = {0, 0};
    mq_agg ag = {};
    if (hipMemcpyAsync(h, d_hdr, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (have_vb && hipMemcpyAsync(&ag, d_agg, sizeof ag, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
        return done(set_err(MQ_EHIP, "%s: header download failed", who));
    if (h[1]) return done(set_err(MQ_EINVAL, "%s: %llu matching rows with a key outside its column's bounds", who, h[1]));
    if (have_vb && (ag.min < vb[0] || ag.max > vb[1]))
        return done(set_err(MQ_EINVAL, "%s: the matching rows' values [%d, %d] leave the bounds [%d, %d]", who, ag.min, ag.max, vb[0], vb[1]));
    // by value, the codes along; then by code, stable, the values along
    va = static_cast<int32_t*>(pool_alloc(k * 4));
    pa = static_cast<uint64_t*>(pool_alloc(k * 8));
    ca = static_cast<int32_t*>(pool_alloc(k * 4));
    if (!va || !pa || !ca) return oom();
    if ((rc = mq_index_build(vals, k, va, pa, stream))) return done(rc);
    if ((rc = mq_gather_u64(packed, pa, k, ca, stream))) return done(rc);
    cs = static_cast<int32_t*>(pool_alloc(k * 4));
    pb = static_cast<uint64_t*>(pool_alloc(k * 8));
    vf = static_cast<int32_t*>(pool_alloc(k * 4));
    if (!cs || !pb || !vf) return oom();
    if ((rc = mq_index_build(ca, k, cs, pb, stream))) return done(rc);
    if ((rc = mq_gather_u64(va, pb, k, vf, stream))) return done(rc);
    uint32_t blocks;
    uint64_t chunk;
    mq_group_sort_geometry(k, &blocks, &chunk);
    if (!(ccnt = static_cast<uint32_t*>(pool_alloc((size_t)blocks * 4)))) return oom();
    if (hipMemsetAsync(d_hdr + 2, 0, 2 * sizeof(u64), st) != hipSuccess) return done(set_err(MQ_EHIP, "%s: memset failed", who));
    hipLaunchKernelGGL(k_gdistinct_heads, dim3(blocks), dim3(kTPB), 0, st, cs, vf, (uint32_t)k, chunk, ccnt, d_hdr + 2);
    u64 t[2] = {0, 0};
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(t, d_hdr + 2, sizeof t, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return done(set_err(MQ_EHIP, "%s: k_gdistinct_heads failed", who));
    g->codes = static_cast<int32_t*>(pool_alloc(t[0] * 4));
    g->counts = static_cast<int32_t*>(pool_alloc(t[0] * 4));
    if (!g->codes || !g->counts) return oom();
    if (hipMemsetAsync(g->counts, 0, t[0] * 4, st) != hipSuccess) return done(set_err(MQ_EHIP, "%s: memset failed", who));
    hipLaunchKernelGGL(k_gdistinct_seg_write, dim3(blocks), dim3(kTPB), 0, st, cs, vf, (uint32_t)k, chunk, ccnt, t[0], g->codes, g->counts);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return done(set_err(MQ_EHIP, "%s: k_gdistinct_seg_write failed", who));
    g->groups = t[0];
    *pairs = t[1];
    return done(MQ_OK);
}

}  // namespace

extern "C" {

uint64_t mq_group_distinct_lds_bytes(void) { return kLdsBytes; }
uint64_t mq_group_distinct_bitmap_bytes(void) { return kBitmapBytes; }

int mq_group_distinct_auto_path(const int32_t* h_key_bounds, int nkeys, const int32_t* h_val_bounds, uint64_t* h_bitmap_bytes) {
    const char* who = "mq_group_distinct_auto_path";
    if (h_bitmap_bytes) *h_bitmap_bytes = 0;
    if (nkeys < 1 || nkeys > kMaxKeys) return set_err(MQ_EINVAL, "%s: nkeys %d outside 1..%d", who, nkeys, kMaxKeys);
    if (!h_key_bounds || !h_val_bounds) return set_err(MQ_EINVAL, "%s: NULL pointer", who);
    Shape sh;
    if (!shape_of(h_key_bounds, nkeys, h_val_bounds, &sh)) return set_err(MQ_EINVAL, "%s: bounds with lo > hi", who);
    if (h_bitmap_bytes) *h_bitmap_bytes = sh.bytes;
    if (sh.space > (1ull << 32)) return set_err(MQ_EINVAL, "%s: the key space %llu is wider than 2^32", who, (u64)sh.space);
    return auto_of(sh);
}

int mq_group_distinct_plan(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols, const int32_t* const* d_keys, int nkeys,
                           const int32_t* d_vals, uint64_t n, const int32_t* h_key_bounds, const int32_t* h_val_bounds, int path,
                           mq_gdistinct** out, uint64_t* h_groups, mq_gdistinct_info* h_info, void* stream) {
    const char* who = "mq_group_distinct_plan";
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (out) *out = nullptr;
    if (h_groups) *h_groups = 0;
    if (h_info) *h_info = mq_gdistinct_info{};
    if (ncols < 0 || ncols > MQ_WHERE_MAX_COLS) return set_err(MQ_EINVAL, "%s: ncols %d outside 0..%d", who, ncols, (int)MQ_WHERE_MAX_COLS);
    if (nkeys < 1 || nkeys > kMaxKeys) return set_err(MQ_EINVAL, "%s: nkeys %d outside 1..%d", who, nkeys, kMaxKeys);
    if (!out || !h_groups || (ncols > 0 && (!d_cols || !h_ranges)) || (n && (!d_keys || !d_vals)))
        return set_err(MQ_EINVAL, "%s: NULL pointer", who);
    if (path != MQ_GDISTINCT_AUTO && path != MQ_GDISTINCT_LDS && path != MQ_GDISTINCT_BITMAP && path != MQ_GDISTINCT_SORT)
        return set_err(MQ_EINVAL, "%s: path %d", who, path);
    if (n >= (1ull << 31)) return set_err(MQ_EINVAL, "%s: n >= 2^31", who);
    int32_t kb[2 * kMaxKeys], vb[2] = {0, 0};
    Shape sh = {};
    // what is known of the bounds, checked before anything is allocated and again once the plan found the rest
    auto check = [&](bool have_k, bool have_v) {
        uint64_t space = 0;
        if (have_k && !group_key_space(kb, nkeys, &space)) return set_err(MQ_EINVAL, "%s: a key column's bounds are empty", who);
        if (have_v && vb[0] > vb[1]) return set_err(MQ_EINVAL, "%s: the value bounds are empty", who);
        if (have_k && space > (1ull << 32))
            return set_err(MQ_EINVAL, "%s: the key space %llu (saturated at 2^63) is wider than 2^32", who, (u64)space);
        if (!have_k || !have_v) return (int)MQ_OK;
        shape_of(kb, nkeys, vb, &sh);
        if (path == MQ_GDISTINCT_LDS && sh.bytes > kLdsBytes)
            return set_err(MQ_EINVAL, "%s: a bitmap of %llu bytes exceeds the LDS path's %llu", who, (u64)sh.bytes, (u64)kLdsBytes);
        if (path == MQ_GDISTINCT_BITMAP && sh.bytes > kBitmapBytes)
            return set_err(MQ_EINVAL, "%s: a bitmap of %llu bytes exceeds the bitmap path's %llu", who, (u64)sh.bytes, (u64)kBitmapBytes);
        return (int)MQ_OK;
    };
    if (n) {
        for (int c = 0; c < ncols; c++)
            if (!d_cols[c] || (reinterpret_cast<uintptr_t>(d_cols[c]) & 3u))
                return set_err(MQ_EINVAL, "%s: column %d NULL or not 4-byte aligned", who, c);
        for (int j = 0; j < nkeys; j++)
            if (!d_keys[j] || (reinterpret_cast<uintptr_t>(d_keys[j]) & 3u))
                return set_err(MQ_EINVAL, "%s: key column %d NULL or not 4-byte aligned", who, j);
        if (reinterpret_cast<uintptr_t>(d_vals) & 3u) return set_err(MQ_EINVAL, "%s: value column not 4-byte aligned", who);
        if (h_key_bounds)
            for (int j = 0; j < 2 * nkeys; j++) kb[j] = h_key_bounds[j];
        if (h_val_bounds) vb[0] = h_val_bounds[0], vb[1] = h_val_bounds[1];
        if ((rc = check(h_key_bounds != nullptr, h_val_bounds != nullptr))) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    int dev = -1;
    if ((rc = current_device(&dev))) return rc;
    WhereArgs w;
    bool empty, vec;
    fold_ranges(d_cols, h_ranges, ncols, &w, &empty, &vec);
    mq_gdistinct* g = new (std::nothrow) mq_gdistinct();
    if (!g) return set_err(MQ_ENOMEM, "%s: out of host memory", who);
    g->dev = dev;
    g->nkeys = nkeys;
    g->stream = st;
    mq_gdistinct_info info = {};
    info.path = path != MQ_GDISTINCT_AUTO ? path : MQ_GDISTINCT_LDS;  // what a plan without rows reports
    auto finish = [&]() {
        if (h_info) *h_info = info;
        *h_groups = g->groups;
        *out = g;
        return MQ_OK;
    };
    auto fail = [&](int code) {
        release(g, st);
        return code;
    };
    if (n == 0 || empty) return finish();
    if (!h_key_bounds || !h_val_bounds) {  // the missing bounds: one more pass each
        const size_t ws_bytes = ncols ? mq_where_workspace_bytes(n) : mq_scan_workspace_bytes(0);
        char* ws = static_cast<char*>(pool_alloc(ws_bytes));
        mq_agg* d_agg = static_cast<mq_agg*>(pool_alloc((kMaxKeys + 1) * sizeof(mq_agg)));
        mq_agg ag[kMaxKeys + 1] = {};
        rc = ws && d_agg ? MQ_OK : set_err(MQ_ENOMEM, "%s: workspace allocation failed", who);
        uint64_t found = n;
        if (!rc && !h_key_bounds && ncols) {
            bool kvec = vec;
            for (int j = 0; j < nkeys; j++) kvec = kvec && aligned16(d_keys[j]);
            rc = group_where_key_bounds(s, w, kvec, d_keys, nkeys, n, &found, kb, st, who);  // synchronises
        }
        if (!rc && found) {
            int q = 0;
            if (!h_key_bounds && !ncols)
                for (int j = 0; j < nkeys && !rc; j++) rc = mq_reduce(d_keys[j], n, d_agg + q++, ws, ws_bytes, stream);
            if (!rc && !h_val_bounds)
                rc = ncols ? mq_where_agg(d_cols, h_ranges, ncols, d_vals, n, d_agg + q, ws, ws_bytes, stream)
                           : mq_reduce(d_vals, n, d_agg + q, ws, ws_bytes, stream);
            if (!rc && hipMemcpyAsync(ag, d_agg, sizeof ag, hipMemcpyDeviceToHost, st) != hipSuccess)
                rc = set_err(MQ_EHIP, "%s: bounds download failed", who);
            if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = set_err(MQ_EHIP, "%s: stream failed", who);
            if (!rc && !h_key_bounds && !ncols)
                for (int j = 0; j < nkeys; j++) kb[2 * j] = ag[j].min, kb[2 * j + 1] = ag[j].max;
            if (!rc && !h_val_bounds) {
                found = ag[q].count;
                vb[0] = ag[q].min;
                vb[1] = ag[q].max;
            }
        }
        pool_free(ws);
        pool_free(d_agg);
        if (rc) return fail(rc);
        if (found == 0) return finish();  // no matching row
        if ((rc = check(true, true))) return fail(rc);
    }
    const int taken = path != MQ_GDISTINCT_AUTO ? path : auto_of(sh);
    ByArgs a = {};
    uint64_t stride = 1;  // up to the key space
    for (int j = nkeys - 1; j >= 0; j--) {
        a.keys[j] = d_keys[j];
        a.lo[j] = (uint32_t)kb[2 * j];
        a.rm1[j] = (uint32_t)((int64_t)kb[2 * j + 1] - (int64_t)kb[2 * j]);
        a.stride[j] = (uint32_t)stride;
        g->klo[j] = kb[2 * j];
        g->krm1[j] = a.rm1[j];
        g->kstride[j] = a.stride[j];
        stride *= (uint64_t)a.rm1[j] + 1;
    }
    uint64_t rows = 0, pairs = 0;
    if (taken == MQ_GDISTINCT_SORT) {
        rc = plan_sort(s, g, d_cols, h_ranges, ncols, a, d_vals, h_val_bounds != nullptr, vb, n, &rows, &pairs, st);
    } else {
        bool mvec = vec && aligned16(d_vals);
        for (int j = 0; j < nkeys; j++) mvec = mvec && aligned16(d_keys[j]);
        rc = plan_bitmap(s, g, taken == MQ_GDISTINCT_LDS, w, mvec, a, d_vals, vb[0], sh, n, &rows, &pairs, st);
    }
    if (rc) return fail(rc);
    info.path = taken;
    info.space = sh.space;
    info.span = sh.span;
    info.bitmap_bytes = taken == MQ_GDISTINCT_SORT ? 0 : sh.bytes;
    info.rows = rows;
    info.pairs = pairs;
    return finish();
}

int mq_group_distinct_write(mq_gdistinct* g, int32_t* const* d_keys_out, uint64_t* d_distinct_out, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!g) return set_err(MQ_EINVAL, "mq_group_distinct_write: NULL handle");
    int dev = -1;
    if ((rc = current_device(&dev))) return rc;
    if (dev != g->dev) return set_err(MQ_EINVAL, "mq_group_distinct_write: the plan was made on device %d", g->dev);
    if (g->groups == 0) return MQ_OK;
    hipStream_t st = (hipStream_t)stream;
    g->stream = st;
    int32_t* keys[kMaxKeys] = {};
    bool want = false;
    for (int j = 0; j < g->nkeys; j++) {
        keys[j] = d_keys_out ? d_keys_out[j] : nullptr;
        want = want || keys[j];
    }
    const uint32_t grid = stream_grid(s, g->groups);
    if (want) group_launch_unpack(g->codes, g->groups, g->klo, g->krm1, g->kstride, g->nkeys, 0u, keys, grid, st);
    if (d_distinct_out)
        hipLaunchKernelGGL(k_gdistinct_widen, dim3(grid), dim3(kTPB), 0, st, g->counts, (u64)g->groups, reinterpret_cast<u64*>(d_distinct_out));
    LAUNCHCHK("k_group_by_unpack / k_gdistinct_widen");
    return MQ_OK;
}

int mq_group_distinct_free(mq_gdistinct* g) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!g) return MQ_OK;
    release(g, g->stream);  // a queued write may still read the buffers: freed in its stream's order
    return MQ_OK;
}

}  // extern "C"
