// mq_where_common.h — internal (not exported) pieces shared by the kernels that stream
// under a conjunction of range predicates (mq_where.hip, k_group_where_dense in
// mq_group.hip): the folded predicates as kernel arguments, a lane's surviving rows per
// tile with the dead 128-byte lines of the later columns skipped, and the host's fold; the
// key set that mq_keyset.hip builds and mq_where.hip's semi-join kernels probe; and the key
// map that mq_keymap.hip builds on it and k_group_join_dense in mq_group.hip looks up; and the
// terms of a star query (k_star_mask in mq_where.hip, k_group_star_dense in mq_group.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mq_common.h"
#include "mq_device.h"
#include "mq_scan_common.h"

namespace mqi {

struct WhereArgs {
    const int32_t* col[MQ_WHERE_MAX_COLS];
    uint32_t lo[MQ_WHERE_MAX_COLS];   // Pred's fold: v matches when (uint32)(v - lo) <= wm1
    uint32_t wm1[MQ_WHERE_MAX_COLS];
    int ncols;                        // predicates that read a column: 0 .. MQ_WHERE_MAX_COLS
};

// The lane's four rows as a nibble: bit e set when row e is in range.
__device__ __forceinline__ uint32_t match4(int4 v, uint32_t lo, uint32_t wm1) {
    return (uint32_t)((uint32_t)v.x - lo <= wm1) | ((uint32_t)((uint32_t)v.y - lo <= wm1) << 1) |
           ((uint32_t)((uint32_t)v.z - lo <= wm1) << 2) | ((uint32_t)((uint32_t)v.w - lo <= wm1) << 3);
}

// Whether one of the 8 lanes that share this lane's 128-byte line is set in the ballot.
__device__ __forceinline__ bool line_live(unsigned long long ballot, int lane) {
    return ((ballot >> (lane & 56)) & 0xffull) != 0;
}

// live[u] = the surviving rows of U full tiles (lane's rows `row` + u * kTileRows .. + 3).
template <bool VEC, int U>
__device__ __forceinline__ void live_tiles(const WhereArgs& a, uint64_t row, int lane, uint32_t (&live)[U]) {
    if (a.ncols == 0) {  // every range matches everything
#pragma unroll
        for (int u = 0; u < U; u++) live[u] = 15u;
        return;
    }
    int4 v[U];
    {
        const int32_t* __restrict__ p = a.col[0] + row;
#pragma unroll
        for (int u = 0; u < U; u++) v[u] = load4_nt<VEC>(p + (uint64_t)u * kTileRows);
        const uint32_t lo = a.lo[0], wm1 = a.wm1[0];
#pragma unroll
        for (int u = 0; u < U; u++) live[u] = match4(v[u], lo, wm1);
    }
    for (int c = 1; c < a.ncols; c++) {
        unsigned long long b[U];
        unsigned long long any = 0;
#pragma unroll
        for (int u = 0; u < U; u++) {
            b[u] = __ballot(live[u] != 0u);
            any |= b[u];
        }
        if (any == 0) break;  // wave-uniform: nothing left in the iteration
        const int32_t* __restrict__ p = a.col[c] + row;
#pragma unroll
        for (int u = 0; u < U; u++)
            if (b[u] != 0 && line_live(b[u], lane)) v[u] = load4_nt<VEC>(p + (uint64_t)u * kTileRows);
        const uint32_t lo = a.lo[c], wm1 = a.wm1[c];
#pragma unroll
        for (int u = 0; u < U; u++)
            if (b[u] != 0 && line_live(b[u], lane)) live[u] &= match4(v[u], lo, wm1);
    }
}

// The column's last, ragged tile: row by row, no row at or past `end` from any column.
__device__ __forceinline__ uint32_t live_ragged(const WhereArgs& a, uint64_t row, uint64_t end) {
    uint32_t live = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        if (row + e >= end) continue;
        bool ok = true;
        for (int c = 0; c < a.ncols && ok; c++) ok = (uint32_t)a.col[c][row + e] - a.lo[c] <= a.wm1[c];
        live |= (uint32_t)ok << e;
    }
    return live;
}

// The key set's lookup as kernel arguments (mq_where.hip's k_semi_*): key k is in the set
// when d = (uint32)(k - lo) <= wm1 and bit d of `bits` is set.
struct SemiArgs {
    const int32_t* key;
    const uint32_t* bits;
    uint32_t lo, wm1;
    uint32_t vec16;  // the bitmap in 16-byte pieces (what an LDS block copies)
    uint32_t flip;   // 0: semi (key IN set); 15: anti (key NOT IN set), xor'ed onto the hit nibble
};

// The key map's lookup as kernel arguments (mq_keymap.hip, k_group_join_dense): key k has a
// partner when d = (uint32)(k - lo) <= wm1 and bit d & 31 of the low half of e = dir[d >> 5] is
// set; its attribute is attr[(e >> 32) + popc(low(e) & ((1 << (d & 31)) - 1))].
struct MapArgs {
    const int32_t* key;
    const unsigned long long* dir;
    const int32_t* attr;
    uint32_t lo, wm1;
};

// The directory entry of offset d, or 0 (no bit set) for a key outside the span.
__device__ __forceinline__ unsigned long long map_entry(const MapArgs& m, uint32_t d) {
    return d <= m.wm1 ? m.dir[d >> 5] : 0ull;
}
__device__ __forceinline__ bool map_hit(unsigned long long e, uint32_t d) { return ((uint32_t)e >> (d & 31u)) & 1u; }
__device__ __forceinline__ uint32_t map_rank(unsigned long long e, uint32_t d) {
    return (uint32_t)(e >> 32) + (uint32_t)__popc((uint32_t)e & ((1u << (d & 31u)) - 1u));
}

// One term of a star query (mq_star_positions, mq_group_star_plan) as kernel arguments: a fact
// column and what its value means. kStarSet: the row is kept when the value is in the key set
// `bits` over [klo, klo + kwm1] (SemiArgs' lookup); no component. kStarMap: the row is kept when
// the value is a key of the map (MapArgs' lookup on dir / attr; `bits` is the map's own key set
// bitmap, which the mask kernel probes instead of the directory) and its attribute is the
// component. kStarPlain: no condition, the value is the component. A component c adds
// (c - lo) * stride to the row's tuple code and is in bounds when (uint32)(c - lo) <= rm1
// (ByArgs' rule, per component).
enum : uint32_t { kStarPlain = 0, kStarMap = 1, kStarSet = 2 };

struct StarTerm {
    const int32_t* col;
    const uint32_t* bits;
    const unsigned long long* dir;
    const int32_t* attr;
    uint32_t klo, kwm1;
    uint32_t lo, rm1, stride;
    uint32_t kind;
};

struct StarArgs {
    StarTerm t[MQ_STAR_MAX_TERMS];
    int nterms;
};

// The term's map as MapArgs (map_entry, map_hit and map_rank serve it).
__device__ __forceinline__ MapArgs star_map(const StarTerm& t) { return MapArgs{t.col, t.dir, t.attr, t.klo, t.kwm1}; }

// The bitmap word of offset d, or 0 (no bit set) for a key outside the span.
__device__ __forceinline__ uint32_t star_word(const StarTerm& t, uint32_t d) { return d <= t.kwm1 ? t.bits[d >> 5] : 0u; }

// The host's fold of ncols checked (column, range) pairs into *a. A range that matches
// every int32 drops out (its column is not read). *empty: some range matches no int32 (*a
// is then incomplete); *vec: every column that is read lies on a 16-byte boundary.
inline void fold_ranges(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols, WhereArgs* a, bool* empty,
                        bool* vec) {
    *a = WhereArgs{};
    *empty = false;
    *vec = true;
    for (int c = 0; c < ncols; c++) {
        Pred p;
        if (!make_pred(h_ranges[c].has_low, h_ranges[c].low, h_ranges[c].has_high, h_ranges[c].high, &p)) {
            *empty = true;
            return;
        }
        if (p.wm1 == 0xFFFFFFFFu) continue;  // matches every int32: the column is not read
        a->col[a->ncols] = d_cols[c];
        a->lo[a->ncols] = p.lo;
        a->wm1[a->ncols] = p.wm1;
        a->ncols++;
        *vec = *vec && aligned16(d_cols[c]);
    }
}

}  // namespace mqi

// A key set (mq_keyset_build in mq_keyset.hip, probed by mq_semi_* in mq_where.hip): one bit
// per value of [lo, hi], immutable once built.
struct mq_keyset {
    int dev;
    int32_t lo, hi;     // lo > hi: the empty set (bits == nullptr)
    uint64_t distinct;
    uint64_t bytes;     // of the bitmap: a multiple of 16, the padding zero
    uint32_t* bits;     // pool_alloc'd
};

// A key map (mq_keymap_build in mq_keymap.hip): a key set over the dimension's primary key,
// its rank directory and the attributes in key order; immutable once built.
struct mq_keymap {
    mq_keyset* ks;            // owned; lo > hi: the empty map (dir == attr == nullptr)
    unsigned long long* dir;  // one entry per 32 keys of the span (per bitmap word, padding included):
                              // low half the bitmap word, high half the set bits of all earlier words
    int32_t* attr;            // attr_by_rank[n1]
    int32_t attr_lo, attr_hi;
    uint64_t n1;
    uint64_t bytes;           // bitmap + directory + attributes
};
