// mq_group.hip — grouped count / sum / min / max by an int32 key.
//
// n rows of (key, value), both int32, give one entry per distinct key in ascending
// signed key order: the key, its row count (u64), the exact int64 sum of its values and
// their min / max. The reference has no such operator; the semantics are restated in
// numpy by tests/groupcases.py. Every combine is an integer add / min / max, so the
// result does not depend on the order in which blocks, waves or lanes contribute.
//
// A plan and a write on a handle (the caller sizes the outputs from the plan's group
// count), by one of two paths chosen from the key range hi - lo + 1 alone:
//
// dense (range <= kDenseSlots), one streaming read of both columns:
//   k_group_dense      : k_scan's chunking and nt dwordx4 loads, kGrpU tiles of each
//                        column in flight. Each block keeps a table in LDS addressed by
//                        key - lo, as four arrays (u32 count, u64 sum, min, max: neighbouring
//                        slots lie in neighbouring banks), updated with LDS atomics. A
//                        wave tile (256 rows) whose keys are all equal is folded into
//                        per-lane registers instead, and the run of such tiles is flushed
//                        with one update when the key changes: a clustered key column and
//                        a one-key column issue a handful of atomics per block. A key
//                        outside [lo, hi] is counted, never used as an address. The block's
//                        table leaves with plain stores to its own slice of the scratch.
//   k_group_fold       : per slot, the sum over the blocks' tables (16 slots x 16 block
//                        strides a workgroup, the strides combined through LDS).
//   k_group_rank       : the non-empty slots' output index (one block scan) and the group
//                        count; also the sum of the blocks' out-of-bounds counts.
//   k_group_dense_write: non-empty slot s goes to out[rank[s]], key lo + s.
//
// sort (everything else): rows ordered by key with mq_index_build (sorted keys and row
// positions, the project's one sort), then
//   k_group_heads      : run heads (sorted[i] != sorted[i - 1]) counted per chunk of a
//                        fixed grid; their total is the group count.
//   k_group_seg_init   : identity into the outputs of the groups that meet a chunk edge.
//   k_group_seg_write  : each block walks its chunk in 1024-row tiles: the rows' group
//                        index follows from the heads before them (chunk sums below, then
//                        ballots), values are gathered through the positions and reduced
//                        per run in LDS. A run inside one tile is stored directly; the run
//                        left open at a tile's end is carried to the next tile; a run that
//                        crosses a chunk edge is combined with atomics onto the identity.
//
// mq_group_where_plan is the same operator over the rows for which a
// conjunction of range predicates holds (mq_where.hip's definition), on the same handle:
//   k_group_where_dense: k_where_agg's stream (mq_where_common.h: the predicate columns,
//                        then of the key and the value column only the 128-byte lines in
//                        which a row survived) feeding k_group_dense's table, rows whose
//                        bit is set only; a wave tile whose surviving rows share one key
//                        (all 256 of them, or the live part of a partly live tile) joins
//                        the run fold. The fold, the rank and the write kernels above
//                        serve it unchanged.
//   sort path          : mq_where_positions, the keys and the values of the K matching rows
//                        gathered with mq_fetch into two buffers, then the sort path above
//                        on them; the handle owns the gathered values.
//
// mq_group_by_plan groups by a tuple of two to four key columns, in
// lexicographic order, on the same handle. With per-column bounds [lo_j, hi_j], ranges
// range_j = hi_j - lo_j + 1 and strides stride_last = 1, stride_j = stride_{j+1} * range_{j+1},
// a tuple's code sum((K_j - lo_j) * stride_j) orders as the tuples do; the key space P =
// prod(range_j) picks the path. Every component is checked against its own range: a stray
// component can leave the summed code inside [0, P).
//   k_group_by_dense   : (P <= kDenseSlots) k_group_dense's stream over the nkeys + 1 columns,
//                        the code as the slot; a row out of bounds takes slot ~0, which no
//                        table holds, and is counted. The run fold keeps tiles whose 256
//                        slots are equal. Fold, rank and write kernels serve unchanged.
//   k_group_by_pack    : (P <= 2^32) reads the key columns once and writes the int32 column
//                        code ^ 0x80000000, whose signed order is the tuples' order; rows out
//                        of bounds are counted per wave (k_group_by_bad sums them). The sort
//                        path above then runs on that column.
//   k_group_by_unpack  : the write kernels put each group's slot or code into a temporary;
//                        this decodes it into the key outputs, K_j = lo_j + (code / stride_j)
//                        % range_j.
//
// mq_group_by_where_plan is mq_group_by_plan over the rows for which a
// conjunction of range predicates holds, on the same handle:
//   k_group_by_where_dense : (P <= kDenseSlots) k_group_where_dense's stream over the
//                        predicate columns and the surviving lines of the nkeys + 1 columns,
//                        k_group_by_dense's code as the slot, live rows only.
//   k_group_by_where_bounds: (no bounds given) every key column's min and max over the
//                        matching rows and their number in one pass, one ByBounds a block;
//                        k_group_by_where_bounds_fold combines them.
//   k_group_by_pack_pos: (P <= 2^32) code ^ 0x80000000 of the K matching rows, read from the
//                        key columns through mq_where_positions' positions; the values are
//                        gathered with mq_fetch and the sort path runs on the K codes.
//
// mq_group_join_plan is mq_group_where_plan with the group key found by a
// key map (mq_keymap.hip: the dimension of an N:1 join as bitmap, rank directory and attributes
// in key order), fact rows without a partner dropped, on the same handle. The attribute range
// is the map's, so no bounds pass reads the fact table:
//   k_group_join_dense : k_group_where_dense's stream with the lookup between the foreign key
//                        column and the tables: the directory entry for surviving rows, the
//                        attribute for hits, and of the value column only the lines that still
//                        hold a joined row.
//   sort path          : mq_semi_positions on the map's key set, the K joined rows' attributes
//                        by mq_keymap_lookup and values by mq_fetch, then the sort path above.
//
// mq_group_star_plan is mq_group_by_where_plan over the rows that every term
// of a star query keeps (mq_where_common.h: StarArgs; a fact column grouped through a key map,
// filtered by a key set, or a group key itself), the tuple made of the maps' attributes and the
// plain columns, on the same handle:
//   k_group_star_dense : (P <= kDenseSlots) k_group_by_where_dense's stream and tables; term by
//                        term the surviving lines of the term's column, the bitmap word or the
//                        directory entry and attribute for surviving rows, the component added
//                        to the row's code and checked against its own bounds.
//   sort path          : mq_star_positions (mq_where.hip) gives the K joined rows,
//                        k_group_star_pack_pos their codes read through the positions, mq_fetch
//                        their values, then the sort path above on the codes.

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

struct mq_group {
    int path;
    int dev;
    uint64_t n, groups;
    const int32_t* vals;
    int32_t* own_vals;   // mq_group_where_plan's sort path: the gathered values (vals points here)
    hipStream_t stream;  // of the last call that queued work on the buffers below
    // dense: the folded table
    int32_t lo;
    uint32_t range;
    char* tab;
    // sort: the sorted keys, their rows, the chunks' head counts
    int32_t* sorted;
    unsigned long long* pos;
    uint32_t* ccnt;
    uint32_t blocks;
    uint64_t chunk;
    // mq_group_by_plan with nkeys > 1 (0 otherwise): the tuple behind a slot (dense, lo = 0) or
    // behind a sorted code, K_j = klo[j] + (code / kstride[j]) % (krm1[j] + 1)
    int nkeys;
    int32_t klo[MQ_GROUP_MAX_KEYS];
    uint32_t krm1[MQ_GROUP_MAX_KEYS];
    uint32_t kstride[MQ_GROUP_MAX_KEYS];
};

namespace {

using namespace mqi;
using u64 = unsigned long long;

// 2048 slots x 20 B = 40 KiB of LDS a block: 4 blocks (16 waves) a CU in 160 KiB.
constexpr uint32_t kDenseSlots = 2048;
constexpr int kGrpU = 4;                       // tiles of each column in flight per thread
constexpr int kGwU = 4;                        // the same under predicates (k_group_where_dense)
constexpr int kGjU = 4;                        // the same with a key map's lookup (k_group_join_dense)
constexpr int kFoldSlots = 16;                 // slots per fold workgroup
constexpr int kFoldParts = kTPB / kFoldSlots;  // block strides per slot
constexpr int kSegBlocks = 2048;               // chunks of the sort path's passes
constexpr int kSegU = 4;                       // rows per lane per tile
constexpr int kSegTile = kTPB * kSegU;

// The sort path's fixed grid over the n sorted rows (k_group_heads, k_group_seg_write).
void seg_chunks(uint64_t n, uint32_t* blocks, uint64_t* chunk) { chunks(n, kSegTile, kSegBlocks, blocks, chunk); }

// The blocks' tables in the scratch, [block][slot] each; bad: [block][wave].
struct DenseTabs {
    long long* sum;
    uint32_t* cnt;
    int* mn;
    int* mx;
    uint32_t* bad;
};

size_t dense_scratch_bytes(uint32_t blocks, uint32_t range) {
    return (size_t)blocks * range * 20 + (size_t)blocks * kWaves * 4;
}

DenseTabs dense_tabs(void* scratch, uint32_t blocks, uint32_t range) {
    const size_t cells = (size_t)blocks * range;
    DenseTabs t;
    t.sum = static_cast<long long*>(scratch);
    t.cnt = reinterpret_cast<uint32_t*>(t.sum + cells);
    t.mn = reinterpret_cast<int*>(t.cnt + cells);
    t.mx = t.mn + cells;
    t.bad = reinterpret_cast<uint32_t*>(t.mx + cells);
    return t;
}

// The folded table in the handle: [groups u64][bad u64] then per slot count, sum, min,
// max and the output index.
struct FinalTab {
    u64* hdr;
    u64* cnt;
    long long* sum;
    int* mn;
    int* mx;
    uint32_t* rank;
};

size_t final_bytes(uint32_t range) { return 16 + (size_t)range * 28; }

FinalTab final_tab(char* p, uint32_t range) {
    FinalTab f;
    f.hdr = reinterpret_cast<u64*>(p);
    f.cnt = f.hdr + 2;
    f.sum = reinterpret_cast<long long*>(f.cnt + range);
    f.mn = reinterpret_cast<int*>(f.sum + range);
    f.mx = f.mn + range;
    f.rank = reinterpret_cast<uint32_t*>(f.mx + range);
    return f;
}

template <bool VK, bool VV>
__global__ __launch_bounds__(kTPB, 4) void k_group_dense(const int* keys, const int* vals, uint64_t n,
                                                         uint64_t rows_per_block, int32_t lo, uint32_t range,
                                                         DenseTabs out) {
    __shared__ uint32_t s_cnt[kDenseSlots];
    __shared__ u64 s_sum[kDenseSlots];
    __shared__ int s_mn[kDenseSlots];
    __shared__ int s_mx[kDenseSlots];
    const int tid = threadIdx.x, lane = tid & 63;
    for (uint32_t s = tid; s < range; s += kTPB) {
        s_cnt[s] = 0u;
        s_sum[s] = 0ull;
        s_mn[s] = INT_MAX;
        s_mx[s] = INT_MIN;
    }
    __syncthreads();
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;

    uint32_t nbad = 0;
    // the wave's run of tiles whose 256 keys all equal run_key, folded per lane
    int run_key = 0;
    uint32_t run_tiles = 0;
    long long r_sum = 0;
    int r_mn = INT_MAX, r_mx = INT_MIN;

    auto update = [&](int k, int v) {
        const uint32_t s = (uint32_t)k - (uint32_t)lo;  // a key below lo wraps past range
        if (s < range) {
            atomicAdd(&s_cnt[s], 1u);
            atomicAdd(&s_sum[s], (u64)(long long)v);
            atomicMin(&s_mn[s], v);
            atomicMax(&s_mx[s], v);
        } else {
            nbad++;
        }
    };
    auto flush = [&]() {  // wave-uniform
        const long long sm = wave_sum_i64(r_sum);
        const int mn = wave_min(r_mn), mx = wave_max(r_mx);
        if (lane == 0) {
            const uint32_t s = (uint32_t)run_key - (uint32_t)lo;
            if (s < range) {
                atomicAdd(&s_cnt[s], run_tiles * 256u);
                atomicAdd(&s_sum[s], (u64)sm);
                atomicMin(&s_mn[s], mn);
                atomicMax(&s_mx[s], mx);
            } else {
                nbad += run_tiles * 256u;
            }
        }
        run_tiles = 0;
        r_sum = 0;
        r_mn = INT_MAX;
        r_mx = INT_MIN;
    };
    auto consume = [&](int4 k, int4 v) {  // a full tile
        const int k0 = __builtin_amdgcn_readfirstlane(k.x);
        if (__all(k.x == k0 && k.y == k0 && k.z == k0 && k.w == k0)) {
            if (run_tiles && k0 != run_key) flush();
            run_key = k0;
            run_tiles++;
            r_sum += (long long)v.x + (long long)v.y + (long long)v.z + (long long)v.w;
            r_mn = min(r_mn, min(min(v.x, v.y), min(v.z, v.w)));
            r_mx = max(r_mx, max(max(v.x, v.y), max(v.z, v.w)));
        } else {
            update(k.x, v.x);
            update(k.y, v.y);
            update(k.z, v.z);
            update(k.w, v.w);
        }
    };

    uint64_t t = start;
    for (; t + (uint64_t)kGrpU * kTileRows <= end; t += (uint64_t)kGrpU * kTileRows) {
        int4 k[kGrpU], v[kGrpU];
#pragma unroll
        for (int u = 0; u < kGrpU; u++) k[u] = load4_nt<VK>(keys + t + (uint64_t)u * kTileRows + (uint64_t)tid * 4);
#pragma unroll
        for (int u = 0; u < kGrpU; u++) v[u] = load4_nt<VV>(vals + t + (uint64_t)u * kTileRows + (uint64_t)tid * 4);
#pragma unroll
        for (int u = 0; u < kGrpU; u++) consume(k[u], v[u]);
    }
    for (; t < end; t += kTileRows) {  // the chunk's tail
        const uint64_t row = t + (uint64_t)tid * 4;
        if (t + kTileRows <= end) {    // block-uniform
            consume(load4_nt<VK>(keys + row), load4_nt<VV>(vals + row));
        } else {                       // the last ragged tile: row by row, none past the end
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (row + e < end) update(keys[row + e], vals[row + e]);
        }
    }
    if (run_tiles) flush();
    nbad = (uint32_t)wave_sum_u64(nbad);
    if (lane == 0) out.bad[(size_t)blockIdx.x * kWaves + (tid >> 6)] = nbad;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * range;
    for (uint32_t s = tid; s < range; s += kTPB) {
        out.cnt[base + s] = s_cnt[s];
        out.sum[base + s] = (long long)s_sum[s];
        out.mn[base + s] = s_mn[s];
        out.mx[base + s] = s_mx[s];
    }
}

// k_group_dense over the rows that survive the predicates of `a`: live_tiles gives each lane
// its rows' nibble per tile, one ballot per tile says which 128-byte lines of the key and the
// value column hold a survivor, and only those are requested (a tile without one issues
// nothing). Keys of rows whose bit is clear are never looked at.
template <bool VEC>
__global__ __launch_bounds__(kTPB, 4) void k_group_where_dense(WhereArgs a, const int* keys, const int* vals, uint64_t n,
                                                               uint64_t rows_per_block, int32_t lo, uint32_t range,
                                                               DenseTabs out) {
    __shared__ uint32_t s_cnt[kDenseSlots];
    __shared__ u64 s_sum[kDenseSlots];
    __shared__ int s_mn[kDenseSlots];
    __shared__ int s_mx[kDenseSlots];
    const int tid = threadIdx.x, lane = tid & 63;
    for (uint32_t s = tid; s < range; s += kTPB) {
        s_cnt[s] = 0u;
        s_sum[s] = 0ull;
        s_mn[s] = INT_MAX;
        s_mx[s] = INT_MIN;
    }
    __syncthreads();
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;

    uint32_t nbad = 0;  // live rows only
    // the wave's run of tiles whose surviving rows all share run_key, folded per lane
    int run_key = 0;
    bool run_open = false;  // wave-uniform
    uint32_t r_cnt = 0;
    long long r_sum = 0;
    int r_mn = INT_MAX, r_mx = INT_MIN;

    auto update = [&](int k, int v) {
        const uint32_t s = (uint32_t)k - (uint32_t)lo;  // a key below lo wraps past range
        if (s < range) {
            atomicAdd(&s_cnt[s], 1u);
            atomicAdd(&s_sum[s], (u64)(long long)v);
            atomicMin(&s_mn[s], v);
            atomicMax(&s_mx[s], v);
        } else {
            nbad++;
        }
    };
    auto flush = [&]() {  // wave-uniform
        const uint32_t c = (uint32_t)wave_sum_u64(r_cnt);  // <= the rows of the block's chunk < 2^31
        const long long sm = wave_sum_i64(r_sum);
        const int mn = wave_min(r_mn), mx = wave_max(r_mx);
        if (lane == 0) {
            const uint32_t s = (uint32_t)run_key - (uint32_t)lo;
            if (s < range) {
                atomicAdd(&s_cnt[s], c);
                atomicAdd(&s_sum[s], (u64)sm);
                atomicMin(&s_mn[s], mn);
                atomicMax(&s_mx[s], mx);
            } else {
                nbad += c;
            }
        }
        run_open = false;
        r_cnt = 0;
        r_sum = 0;
        r_mn = INT_MAX;
        r_mx = INT_MIN;
    };
    // A full tile with a survivor in the wave (b: the lanes that hold one); k and v are loaded
    // in the lanes whose line is live, so in every lane with a bit set.
    auto consume = [&](int4 k, int4 v, uint32_t live, u64 b) {
        const int kf = live & 1u ? k.x : live & 2u ? k.y : live & 4u ? k.z : k.w;  // the lane's first surviving key
        const int k0 = __builtin_amdgcn_readlane(kf, __builtin_ctzll(b));
        const bool same = live == 0u || ((!(live & 1u) || k.x == k0) && (!(live & 2u) || k.y == k0) &&
                                         (!(live & 4u) || k.z == k0) && (!(live & 8u) || k.w == k0));
        if (__all(same)) {  // the surviving rows of the wave's 256 share one key: into the run
            if (run_open && k0 != run_key) flush();
            run_key = k0;
            run_open = true;
            r_cnt += (uint32_t)__popc(live);
            r_sum += (live & 1u ? (long long)v.x : 0ll) + (live & 2u ? (long long)v.y : 0ll) +
                     (live & 4u ? (long long)v.z : 0ll) + (live & 8u ? (long long)v.w : 0ll);
            r_mn = min(r_mn, min(min(live & 1u ? v.x : INT_MAX, live & 2u ? v.y : INT_MAX),
                                 min(live & 4u ? v.z : INT_MAX, live & 8u ? v.w : INT_MAX)));
            r_mx = max(r_mx, max(max(live & 1u ? v.x : INT_MIN, live & 2u ? v.y : INT_MIN),
                                 max(live & 4u ? v.z : INT_MIN, live & 8u ? v.w : INT_MIN)));
        } else if (__all(live == 15u)) {  // k_group_dense's tile
            update(k.x, v.x);
            update(k.y, v.y);
            update(k.z, v.z);
            update(k.w, v.w);
        } else {
            if (live & 1u) update(k.x, v.x);
            if (live & 2u) update(k.y, v.y);
            if (live & 4u) update(k.z, v.z);
            if (live & 8u) update(k.w, v.w);
        }
    };
    // U full tiles: every key and value load of the iteration is issued before the first use
    auto tiles = [&](auto uc, uint64_t t) {
        constexpr int U = decltype(uc)::value;
        const uint64_t row = t + (uint64_t)tid * 4;
        uint32_t live[U];
        live_tiles<VEC, U>(a, row, lane, live);
        u64 b[U];
        int4 k[U], v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            b[u] = __ballot(live[u] != 0u);
            if (b[u] != 0 && line_live(b[u], lane)) k[u] = load4_nt<VEC>(keys + row + (uint64_t)u * kTileRows);
        }
#pragma unroll
        for (int u = 0; u < U; u++)
            if (b[u] != 0 && line_live(b[u], lane)) v[u] = load4_nt<VEC>(vals + row + (uint64_t)u * kTileRows);
#pragma unroll
        for (int u = 0; u < U; u++)
            if (b[u] != 0) consume(k[u], v[u], live[u], b[u]);  // wave-uniform
    };

    uint64_t t = start;
    for (; t + (uint64_t)kGwU * kTileRows <= end; t += (uint64_t)kGwU * kTileRows)
        tiles(std::integral_constant<int, kGwU>{}, t);
    for (; t + kTileRows <= end; t += kTileRows) tiles(std::integral_constant<int, 1>{}, t);
    if (t < end) {  // the column's ragged tile: row by row, none past the end
        const uint64_t row = t + (uint64_t)tid * 4;
        const uint32_t live = live_ragged(a, row, end);
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (live & (1u << e)) update(keys[row + e], vals[row + e]);
    }
    if (run_open) flush();
    nbad = (uint32_t)wave_sum_u64(nbad);
    if (lane == 0) out.bad[(size_t)blockIdx.x * kWaves + (tid >> 6)] = nbad;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * range;
    for (uint32_t s = tid; s < range; s += kTPB) {
        out.cnt[base + s] = s_cnt[s];
        out.sum[base + s] = (long long)s_sum[s];
        out.mn[base + s] = s_mn[s];
        out.mx[base + s] = s_mx[s];
    }
}

// k_group_where_dense with a key map's lookup (mq_where_common.h: MapArgs) between the key
// column and the tables: of the foreign key column only the lines with a surviving row are
// requested; for surviving rows only, the directory entry, then for hits the attribute;
// live &= hit, the ballot is taken again, and of the value column only the lines that still
// hold a joined row are requested. consume() then runs on the attributes. Within an iteration
// all directory loads are issued, then all attribute loads, then all value loads, before the
// first use. The fact columns pass by non-temporally; directory and attributes are plain cached
// loads, so that they stay in L2 and the Infinity Cache. An attribute outside [lo, lo + range)
// is counted, never used as an address.
template <bool VEC>
__global__ __launch_bounds__(kTPB, 4) void k_group_join_dense(WhereArgs a, MapArgs m, const int* vals, uint64_t n,
                                                              uint64_t rows_per_block, int32_t lo, uint32_t range,
                                                              DenseTabs out) {
    __shared__ uint32_t s_cnt[kDenseSlots];
    __shared__ u64 s_sum[kDenseSlots];
    __shared__ int s_mn[kDenseSlots];
    __shared__ int s_mx[kDenseSlots];
    const int tid = threadIdx.x, lane = tid & 63;
    for (uint32_t s = tid; s < range; s += kTPB) {
        s_cnt[s] = 0u;
        s_sum[s] = 0ull;
        s_mn[s] = INT_MAX;
        s_mx[s] = INT_MIN;
    }
    __syncthreads();
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;

    uint32_t nbad = 0;  // joined rows only
    // the wave's run of tiles whose joined rows all share the attribute run_key, folded per lane
    int run_key = 0;
    bool run_open = false;  // wave-uniform
    uint32_t r_cnt = 0;
    long long r_sum = 0;
    int r_mn = INT_MAX, r_mx = INT_MIN;

    auto update = [&](int k, int v) {
        const uint32_t s = (uint32_t)k - (uint32_t)lo;  // an attribute below lo wraps past range
        if (s < range) {
            atomicAdd(&s_cnt[s], 1u);
            atomicAdd(&s_sum[s], (u64)(long long)v);
            atomicMin(&s_mn[s], v);
            atomicMax(&s_mx[s], v);
        } else {
            nbad++;
        }
    };
    auto flush = [&]() {  // wave-uniform
        const uint32_t c = (uint32_t)wave_sum_u64(r_cnt);  // <= the rows of the block's chunk < 2^31
        const long long sm = wave_sum_i64(r_sum);
        const int mn = wave_min(r_mn), mx = wave_max(r_mx);
        if (lane == 0) {
            const uint32_t s = (uint32_t)run_key - (uint32_t)lo;
            if (s < range) {
                atomicAdd(&s_cnt[s], c);
                atomicAdd(&s_sum[s], (u64)sm);
                atomicMin(&s_mn[s], mn);
                atomicMax(&s_mx[s], mx);
            } else {
                nbad += c;
            }
        }
        run_open = false;
        r_cnt = 0;
        r_sum = 0;
        r_mn = INT_MAX;
        r_mx = INT_MIN;
    };
    // k_group_where_dense's consume: k holds the attributes of the rows whose bit is set
    auto consume = [&](int4 k, int4 v, uint32_t live, u64 b) {
        const int kf = live & 1u ? k.x : live & 2u ? k.y : live & 4u ? k.z : k.w;  // the lane's first joined row
        const int k0 = __builtin_amdgcn_readlane(kf, __builtin_ctzll(b));
        const bool same = live == 0u || ((!(live & 1u) || k.x == k0) && (!(live & 2u) || k.y == k0) &&
                                         (!(live & 4u) || k.z == k0) && (!(live & 8u) || k.w == k0));
        if (__all(same)) {  // the joined rows of the wave's 256 share one attribute: into the run
            if (run_open && k0 != run_key) flush();
            run_key = k0;
            run_open = true;
            r_cnt += (uint32_t)__popc(live);
            r_sum += (live & 1u ? (long long)v.x : 0ll) + (live & 2u ? (long long)v.y : 0ll) +
                     (live & 4u ? (long long)v.z : 0ll) + (live & 8u ? (long long)v.w : 0ll);
            r_mn = min(r_mn, min(min(live & 1u ? v.x : INT_MAX, live & 2u ? v.y : INT_MAX),
                                 min(live & 4u ? v.z : INT_MAX, live & 8u ? v.w : INT_MAX)));
            r_mx = max(r_mx, max(max(live & 1u ? v.x : INT_MIN, live & 2u ? v.y : INT_MIN),
                                 max(live & 4u ? v.z : INT_MIN, live & 8u ? v.w : INT_MIN)));
        } else {
            if (live & 1u) update(k.x, v.x);
            if (live & 2u) update(k.y, v.y);
            if (live & 4u) update(k.z, v.z);
            if (live & 8u) update(k.w, v.w);
        }
    };
    auto tiles = [&](auto uc, uint64_t t) {
        constexpr int U = decltype(uc)::value;
        const uint64_t row = t + (uint64_t)tid * 4;
        uint32_t live[U];
        live_tiles<VEC, U>(a, row, lane, live);
        u64 b[U];
        int4 fk[U], at[U], v[U];
        u64 e[U][4];
#pragma unroll
        for (int u = 0; u < U; u++) {
            b[u] = __ballot(live[u] != 0u);
            fk[u] = make_int4(0, 0, 0, 0);
            if (b[u] != 0 && line_live(b[u], lane)) fk[u] = load4_nt<VEC>(m.key + row + (uint64_t)u * kTileRows);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {  // the directory entries of the surviving rows
            e[u][0] = live[u] & 1u ? map_entry(m, (uint32_t)fk[u].x - m.lo) : 0ull;
            e[u][1] = live[u] & 2u ? map_entry(m, (uint32_t)fk[u].y - m.lo) : 0ull;
            e[u][2] = live[u] & 4u ? map_entry(m, (uint32_t)fk[u].z - m.lo) : 0ull;
            e[u][3] = live[u] & 8u ? map_entry(m, (uint32_t)fk[u].w - m.lo) : 0ull;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {  // live &= hit; the attributes of the joined rows
            const uint32_t d0 = (uint32_t)fk[u].x - m.lo, d1 = (uint32_t)fk[u].y - m.lo, d2 = (uint32_t)fk[u].z - m.lo,
                           d3 = (uint32_t)fk[u].w - m.lo;
            live[u] &= (uint32_t)map_hit(e[u][0], d0) | ((uint32_t)map_hit(e[u][1], d1) << 1) |
                       ((uint32_t)map_hit(e[u][2], d2) << 2) | ((uint32_t)map_hit(e[u][3], d3) << 3);
            at[u] = make_int4(0, 0, 0, 0);
            if (live[u] & 1u) at[u].x = m.attr[map_rank(e[u][0], d0)];
            if (live[u] & 2u) at[u].y = m.attr[map_rank(e[u][1], d1)];
            if (live[u] & 4u) at[u].z = m.attr[map_rank(e[u][2], d2)];
            if (live[u] & 8u) at[u].w = m.attr[map_rank(e[u][3], d3)];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            b[u] = __ballot(live[u] != 0u);
            if (b[u] != 0 && line_live(b[u], lane)) v[u] = load4_nt<VEC>(vals + row + (uint64_t)u * kTileRows);
        }
#pragma unroll
        for (int u = 0; u < U; u++)
            if (b[u] != 0) consume(at[u], v[u], live[u], b[u]);  // wave-uniform
    };

    uint64_t t = start;
    for (; t + (uint64_t)kGjU * kTileRows <= end; t += (uint64_t)kGjU * kTileRows)
        tiles(std::integral_constant<int, kGjU>{}, t);
    for (; t + kTileRows <= end; t += kTileRows) tiles(std::integral_constant<int, 1>{}, t);
    if (t < end) {  // the column's ragged tile: row by row, none past the end
        const uint64_t row = t + (uint64_t)tid * 4;
        const uint32_t live = live_ragged(a, row, end);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (!(live & (1u << i))) continue;
            const uint32_t d = (uint32_t)m.key[row + i] - m.lo;
            const u64 en = map_entry(m, d);
            if (map_hit(en, d)) update(m.attr[map_rank(en, d)], vals[row + i]);
        }
    }
    if (run_open) flush();
    nbad = (uint32_t)wave_sum_u64(nbad);
    if (lane == 0) out.bad[(size_t)blockIdx.x * kWaves + (tid >> 6)] = nbad;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * range;
    for (uint32_t s = tid; s < range; s += kTPB) {
        out.cnt[base + s] = s_cnt[s];
        out.sum[base + s] = (long long)s_sum[s];
        out.mn[base + s] = s_mn[s];
        out.mx[base + s] = s_mx[s];
    }
}

__global__ __launch_bounds__(kTPB) void k_group_fold(DenseTabs in, uint32_t blocks, uint32_t range, FinalTab f) {
    __shared__ u64 p_cnt[kFoldParts][kFoldSlots];
    __shared__ long long p_sum[kFoldParts][kFoldSlots];
    __shared__ int p_mn[kFoldParts][kFoldSlots];
    __shared__ int p_mx[kFoldParts][kFoldSlots];
    const uint32_t sl = threadIdx.x % kFoldSlots, part = threadIdx.x / kFoldSlots;
    const uint32_t s = blockIdx.x * kFoldSlots + sl;
    u64 c = 0;
    long long sm = 0;
    int mn = INT_MAX, mx = INT_MIN;
    if (s < range)
        for (uint32_t b = part; b < blocks; b += kFoldParts) {
            const size_t i = (size_t)b * range + s;
            c += in.cnt[i];
            sm += in.sum[i];
            mn = min(mn, in.mn[i]);
            mx = max(mx, in.mx[i]);
        }
    p_cnt[part][sl] = c;
    p_sum[part][sl] = sm;
    p_mn[part][sl] = mn;
    p_mx[part][sl] = mx;
    __syncthreads();
    if (part == 0 && s < range) {
        for (int p = 1; p < kFoldParts; p++) {
            c += p_cnt[p][sl];
            sm += p_sum[p][sl];
            mn = min(mn, p_mn[p][sl]);
            mx = max(mx, p_mx[p][sl]);
        }
        f.cnt[s] = c;
        f.sum[s] = sm;
        f.mn[s] = mn;
        f.mx[s] = mx;
    }
}

// One block: rank[s] = non-empty slots below s, hdr[0] = their number, hdr[1] = the keys
// the blocks found outside the bounds.
__global__ __launch_bounds__(kTPB) void k_group_rank(FinalTab f, uint32_t range, const uint32_t* __restrict__ bad,
                                                     uint32_t nbad) {
    __shared__ uint32_t s_w[kWaves];
    constexpr uint32_t kPer = kDenseSlots / kTPB;
    const uint32_t s0 = threadIdx.x * kPer;
    uint32_t c = 0;
#pragma unroll
    for (uint32_t e = 0; e < kPer; e++) c += s0 + e < range && f.cnt[s0 + e] != 0;
    uint32_t total;
    uint32_t r = block_excl_scan(c, s_w, &total);
#pragma unroll
    for (uint32_t e = 0; e < kPer; e++)
        if (s0 + e < range) {
            f.rank[s0 + e] = r;
            r += f.cnt[s0 + e] != 0;
        }
    u64 b = 0;
    for (uint32_t i = threadIdx.x; i < nbad; i += kTPB) b += bad[i];
    b = wave_sum_u64(b);
    __shared__ u64 s_b[kWaves];
    if ((threadIdx.x & 63) == 0) s_b[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        f.hdr[0] = total;
        f.hdr[1] = s_b[0] + s_b[1] + s_b[2] + s_b[3];
    }
}

// One block: *rows = the sum of the slots' counts.
__global__ __launch_bounds__(kTPB) void k_group_rows(FinalTab f, uint32_t range, u64* __restrict__ rows) {
    __shared__ u64 s_r[kWaves];
    u64 c = 0;
    for (uint32_t s = threadIdx.x; s < range; s += kTPB) c += f.cnt[s];
    c = wave_sum_u64(c);
    if ((threadIdx.x & 63) == 0) s_r[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) *rows = s_r[0] + s_r[1] + s_r[2] + s_r[3];
}

__global__ __launch_bounds__(kTPB) void k_group_dense_write(FinalTab f, uint32_t range, int32_t lo,
                                                            int32_t* __restrict__ keys_out, u64* __restrict__ count_out,
                                                            long long* __restrict__ sum_out, int32_t* __restrict__ min_out,
                                                            int32_t* __restrict__ max_out) {
    const uint32_t s = blockIdx.x * kTPB + threadIdx.x;
    if (s >= range) return;
    const u64 c = f.cnt[s];
    if (c == 0) return;
    const uint32_t o = f.rank[s];  // < the group count the plan returned
    if (keys_out) keys_out[o] = (int32_t)((uint32_t)lo + s);
    if (count_out) count_out[o] = c;
    if (sum_out) sum_out[o] = f.sum[s];
    if (min_out) min_out[o] = f.mn[s];
    if (max_out) max_out[o] = f.mx[s];
}

// ---- grouping by a tuple of key columns (mq_group_by_plan) ----

constexpr int kMaxKeys = MQ_GROUP_MAX_KEYS;
constexpr uint32_t kNoSlot = ~0u;  // of a row with a component out of bounds: beyond every table

// Tiles of each column in flight per thread: (nkeys + 1) * by_tiles(nkeys) dwordx4 of loaded
// data a lane, 192 B with two and three key columns and 160 B with four.
constexpr int by_tiles(int nkeys) { return nkeys == 2 ? 4 : nkeys == 3 ? 3 : 2; }

struct ByKeysOut {
    int32_t* keys[kMaxKeys];
};

// ByArgs, row_code and tile_codes, the tuple's code, are in mq_group_impl.h (mq_distinct.hip shares them).

// k_group_dense over NK key columns: the slot is the tuple's code (range = the key space, at
// most kDenseSlots), kNoSlot for a row out of bounds, so that a tile of 256 equal tuples is a
// tile of 256 equal slots and the run fold works on slots.
template <int NK, bool VEC>
__global__ __launch_bounds__(kTPB, 4) void k_group_by_dense(ByArgs a, const int* vals, uint64_t n, uint64_t rows_per_block,
                                                            uint32_t range, DenseTabs out) {
    constexpr int U = by_tiles(NK);
    __shared__ uint32_t s_cnt[kDenseSlots];
    __shared__ u64 s_sum[kDenseSlots];
    __shared__ int s_mn[kDenseSlots];
    __shared__ int s_mx[kDenseSlots];
    const int tid = threadIdx.x, lane = tid & 63;
    for (uint32_t s = tid; s < range; s += kTPB) {
        s_cnt[s] = 0u;
        s_sum[s] = 0ull;
        s_mn[s] = INT_MAX;
        s_mx[s] = INT_MIN;
    }
    __syncthreads();
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;

    uint32_t nbad = 0;
    // the wave's run of tiles whose 256 slots all equal run_slot, folded per lane
    uint32_t run_slot = 0;
    uint32_t run_tiles = 0;
    long long r_sum = 0;
    int r_mn = INT_MAX, r_mx = INT_MIN;

    auto update = [&](uint32_t s, int v) {
        if (s < range) {  // kNoSlot never is
            atomicAdd(&s_cnt[s], 1u);
            atomicAdd(&s_sum[s], (u64)(long long)v);
            atomicMin(&s_mn[s], v);
            atomicMax(&s_mx[s], v);
        } else {
            nbad++;
        }
    };
    auto flush = [&]() {  // wave-uniform
        const long long sm = wave_sum_i64(r_sum);
        const int mn = wave_min(r_mn), mx = wave_max(r_mx);
        if (lane == 0) {
            if (run_slot < range) {
                atomicAdd(&s_cnt[run_slot], run_tiles * 256u);
                atomicAdd(&s_sum[run_slot], (u64)sm);
                atomicMin(&s_mn[run_slot], mn);
                atomicMax(&s_mx[run_slot], mx);
            } else {
                nbad += run_tiles * 256u;
            }
        }
        run_tiles = 0;
        r_sum = 0;
        r_mn = INT_MAX;
        r_mx = INT_MIN;
    };
    auto consume = [&](const int4 (&k)[NK], int4 v) {  // a full tile
        uint32_t in;
        const uint4 c = tile_codes<NK>(a, k, &in);
        const uint32_t sx = in & 1u ? c.x : kNoSlot, sy = in & 2u ? c.y : kNoSlot, sz = in & 4u ? c.z : kNoSlot,
                       sw = in & 8u ? c.w : kNoSlot;
        const uint32_t s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)sx);
        if (__all(sx == s0 && sy == s0 && sz == s0 && sw == s0)) {
            if (run_tiles && s0 != run_slot) flush();
            run_slot = s0;
            run_tiles++;
            r_sum += (long long)v.x + (long long)v.y + (long long)v.z + (long long)v.w;
            r_mn = min(r_mn, min(min(v.x, v.y), min(v.z, v.w)));
            r_mx = max(r_mx, max(max(v.x, v.y), max(v.z, v.w)));
        } else {
            update(sx, v.x);
            update(sy, v.y);
            update(sz, v.z);
            update(sw, v.w);
        }
    };

    uint64_t t = start;
    for (; t + (uint64_t)U * kTileRows <= end; t += (uint64_t)U * kTileRows) {
        int4 k[U][NK], v[U];
#pragma unroll
        for (int j = 0; j < NK; j++)
#pragma unroll
            for (int u = 0; u < U; u++) k[u][j] = load4_nt<VEC>(a.keys[j] + t + (uint64_t)u * kTileRows + (uint64_t)tid * 4);
#pragma unroll
        for (int u = 0; u < U; u++) v[u] = load4_nt<VEC>(vals + t + (uint64_t)u * kTileRows + (uint64_t)tid * 4);
#pragma unroll
        for (int u = 0; u < U; u++) consume(k[u], v[u]);
    }
    for (; t < end; t += kTileRows) {  // the chunk's tail
        const uint64_t row = t + (uint64_t)tid * 4;
        if (t + kTileRows <= end) {    // block-uniform
            int4 k[NK];
#pragma unroll
            for (int j = 0; j < NK; j++) k[j] = load4_nt<VEC>(a.keys[j] + row);
            consume(k, load4_nt<VEC>(vals + row));
        } else {                       // the last ragged tile: row by row, none past the end
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (row + e < end) {
                    int r[NK];
#pragma unroll
                    for (int j = 0; j < NK; j++) r[j] = a.keys[j][row + e];
                    bool ok;
                    const uint32_t c = row_code<NK>(a, r, &ok);
                    update(ok ? c : kNoSlot, vals[row + e]);
                }
        }
    }
    if (run_tiles) flush();
    nbad = (uint32_t)wave_sum_u64(nbad);
    if (lane == 0) out.bad[(size_t)blockIdx.x * kWaves + (tid >> 6)] = nbad;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * range;
    for (uint32_t s = tid; s < range; s += kTPB) {
        out.cnt[base + s] = s_cnt[s];
        out.sum[base + s] = (long long)s_sum[s];
        out.mn[base + s] = s_mn[s];
        out.mx[base + s] = s_mx[s];
    }
}

// out[i] = code(row i) ^ 0x80000000 over n rows, k_group_dense's chunking; bad[block][wave] =
// the rows with a component out of bounds (their out entry means nothing: the plan fails).
// out is 16-byte aligned (a pool block), so a lane's four codes leave as one dwordx4.
template <int NK, bool VEC>
__global__ __launch_bounds__(kTPB) void k_group_by_pack(ByArgs a, uint64_t n, uint64_t rows_per_block, int32_t* __restrict__ out,
                                                        uint32_t* __restrict__ bad) {
    constexpr int U = by_tiles(NK);
    const int tid = threadIdx.x, lane = tid & 63;
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;
    uint32_t nbad = 0;
    auto pack = [&](const int4 (&k)[NK], uint64_t row) {  // a full tile; row < end, a multiple of 4
        uint32_t in;
        const uint4 c = tile_codes<NK>(a, k, &in);
        nbad += 4u - (uint32_t)__popc(in);
        *reinterpret_cast<int4*>(out + row) = make_int4((int)(c.x ^ 0x80000000u), (int)(c.y ^ 0x80000000u),
                                                        (int)(c.z ^ 0x80000000u), (int)(c.w ^ 0x80000000u));
    };
    uint64_t t = start;
    for (; t + (uint64_t)U * kTileRows <= end; t += (uint64_t)U * kTileRows) {
        int4 k[U][NK];
#pragma unroll
        for (int j = 0; j < NK; j++)
#pragma unroll
            for (int u = 0; u < U; u++) k[u][j] = load4_nt<VEC>(a.keys[j] + t + (uint64_t)u * kTileRows + (uint64_t)tid * 4);
#pragma unroll
        for (int u = 0; u < U; u++) pack(k[u], t + (uint64_t)u * kTileRows + (uint64_t)tid * 4);
    }
    for (; t < end; t += kTileRows) {  // the chunk's tail
        const uint64_t row = t + (uint64_t)tid * 4;
        if (t + kTileRows <= end) {    // block-uniform
            int4 k[NK];
#pragma unroll
            for (int j = 0; j < NK; j++) k[j] = load4_nt<VEC>(a.keys[j] + row);
            pack(k, row);
        } else {                       // the last ragged tile: row by row, none past the end
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (row + e < end) {
                    int r[NK];
#pragma unroll
                    for (int j = 0; j < NK; j++) r[j] = a.keys[j][row + e];
                    bool ok;
                    const uint32_t c = row_code<NK>(a, r, &ok);
                    nbad += ok ? 0u : 1u;
                    out[row + e] = (int)(c ^ 0x80000000u);
                }
        }
    }
    nbad = (uint32_t)wave_sum_u64(nbad);
    if (lane == 0) bad[(size_t)blockIdx.x * kWaves + (tid >> 6)] = nbad;
}

// One block: *total = the sum of k_group_by_pack's counts.
__global__ __launch_bounds__(kTPB) void k_group_by_bad(const uint32_t* __restrict__ bad, uint32_t nbad, u64* __restrict__ total) {
    __shared__ u64 s_b[kWaves];
    u64 b = 0;
    for (uint32_t i = threadIdx.x; i < nbad; i += kTPB) b += bad[i];
    b = wave_sum_u64(b);
    if ((threadIdx.x & 63) == 0) s_b[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) *total = s_b[0] + s_b[1] + s_b[2] + s_b[3];
}

// codes[i] ^ flip is group i's code (flip: 0 for the dense path's slots, 0x80000000 for the
// sorted column); component j goes to o.keys[j][i] where that is wanted. A range of one needs
// no division (and its stride may be the 2^32 that a.stride holds as 0); every other
// component's stride is at most 2^31.
__global__ __launch_bounds__(kTPB) void k_group_by_unpack(const int32_t* __restrict__ codes, u64 groups, ByArgs a, int nkeys,
                                                          uint32_t flip, ByKeysOut o) {
    for (u64 i = (u64)blockIdx.x * kTPB + threadIdx.x; i < groups; i += (u64)gridDim.x * kTPB) {
        const uint32_t c = (uint32_t)codes[i] ^ flip;
#pragma unroll
        for (int j = 0; j < kMaxKeys; j++) {
            if (j >= nkeys || !o.keys[j]) continue;
            uint32_t d = 0;
            if (a.rm1[j] != 0u) {
                d = c / a.stride[j];
                if (a.rm1[j] != ~0u) d %= a.rm1[j] + 1u;
            }
            o.keys[j][i] = (int32_t)(a.lo[j] + d);
        }
    }
}

// ---- a tuple of key columns under predicates (mq_group_by_where_plan) ----

// Tiles in flight per thread under predicates: by_tiles' (nkeys + 1) * U dwordx4 of loaded
// data a lane, with the live nibbles beside them (the ballots are scalar).
constexpr int bw_tiles(int nkeys) { return by_tiles(nkeys); }

// k_group_by_dense over the rows that survive the predicates of `w`, k_group_where_dense's
// stream: of the NK key columns and the value column only the 128-byte lines that hold a
// survivor are requested. A row whose bit is clear has nothing loaded behind it in a dead line
// and anything at all in a live one: its code and its bounds bit are never used.
template <int NK, bool VEC>
__global__ __launch_bounds__(kTPB, 4) void k_group_by_where_dense(WhereArgs w, ByArgs a, const int* vals, uint64_t n,
                                                                  uint64_t rows_per_block, uint32_t range, DenseTabs out) {
    constexpr int U = bw_tiles(NK);
    __shared__ uint32_t s_cnt[kDenseSlots];
    __shared__ u64 s_sum[kDenseSlots];
    __shared__ int s_mn[kDenseSlots];
    __shared__ int s_mx[kDenseSlots];
    const int tid = threadIdx.x, lane = tid & 63;
    for (uint32_t s = tid; s < range; s += kTPB) {
        s_cnt[s] = 0u;
        s_sum[s] = 0ull;
        s_mn[s] = INT_MAX;
        s_mx[s] = INT_MIN;
    }
    __syncthreads();
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;

    uint32_t nbad = 0;  // live rows only
    // the wave's run of tiles whose surviving rows all share run_slot, folded per lane
    uint32_t run_slot = 0;
    bool run_open = false;  // wave-uniform
    uint32_t r_cnt = 0;
    long long r_sum = 0;
    int r_mn = INT_MAX, r_mx = INT_MIN;

    auto update = [&](uint32_t s, int v) {
        if (s < range) {  // kNoSlot never is
            atomicAdd(&s_cnt[s], 1u);
            atomicAdd(&s_sum[s], (u64)(long long)v);
            atomicMin(&s_mn[s], v);
            atomicMax(&s_mx[s], v);
        } else {
            nbad++;
        }
    };
    auto flush = [&]() {  // wave-uniform
        const uint32_t c = (uint32_t)wave_sum_u64(r_cnt);  // <= the rows of the block's chunk < 2^31
        const long long sm = wave_sum_i64(r_sum);
        const int mn = wave_min(r_mn), mx = wave_max(r_mx);
        if (lane == 0) {
            if (run_slot < range) {
                atomicAdd(&s_cnt[run_slot], c);
                atomicAdd(&s_sum[run_slot], (u64)sm);
                atomicMin(&s_mn[run_slot], mn);
                atomicMax(&s_mx[run_slot], mx);
            } else {
                nbad += c;
            }
        }
        run_open = false;
        r_cnt = 0;
        r_sum = 0;
        r_mn = INT_MAX;
        r_mx = INT_MIN;
    };
    // A full tile with a survivor in the wave (b: the lanes that hold one); k and v are loaded
    // in the lanes whose line is live, so in every lane with a bit set.
    auto consume = [&](const int4 (&k)[NK], int4 v, uint32_t live, u64 b) {
        uint32_t in;
        const uint4 c = tile_codes<NK>(a, k, &in);  // of a dead row: never read below
        const uint32_t sx = in & 1u ? c.x : kNoSlot, sy = in & 2u ? c.y : kNoSlot, sz = in & 4u ? c.z : kNoSlot,
                       sw = in & 8u ? c.w : kNoSlot;
        const uint32_t sf = live & 1u ? sx : live & 2u ? sy : live & 4u ? sz : sw;  // the lane's first surviving slot
        const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)sf, __builtin_ctzll(b));
        const bool same = live == 0u || ((!(live & 1u) || sx == s0) && (!(live & 2u) || sy == s0) &&
                                         (!(live & 4u) || sz == s0) && (!(live & 8u) || sw == s0));
        if (__all(same)) {  // the surviving rows of the wave's 256 share one slot: into the run
            if (run_open && s0 != run_slot) flush();
            run_slot = s0;
            run_open = true;
            r_cnt += (uint32_t)__popc(live);
            r_sum += (live & 1u ? (long long)v.x : 0ll) + (live & 2u ? (long long)v.y : 0ll) +
                     (live & 4u ? (long long)v.z : 0ll) + (live & 8u ? (long long)v.w : 0ll);
            r_mn = min(r_mn, min(min(live & 1u ? v.x : INT_MAX, live & 2u ? v.y : INT_MAX),
                                 min(live & 4u ? v.z : INT_MAX, live & 8u ? v.w : INT_MAX)));
            r_mx = max(r_mx, max(max(live & 1u ? v.x : INT_MIN, live & 2u ? v.y : INT_MIN),
                                 max(live & 4u ? v.z : INT_MIN, live & 8u ? v.w : INT_MIN)));
        } else {
            if (live & 1u) update(sx, v.x);
            if (live & 2u) update(sy, v.y);
            if (live & 4u) update(sz, v.z);
            if (live & 8u) update(sw, v.w);
        }
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
        for (int u = 0; u < T; u++) b[u] = __ballot(live[u] != 0u);
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
            if (b[u] != 0) consume(k[u], v[u], live[u], b[u]);  // wave-uniform
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
                update(ok ? c : kNoSlot, vals[row + e]);
            }
    }
    if (run_open) flush();
    nbad = (uint32_t)wave_sum_u64(nbad);
    if (lane == 0) out.bad[(size_t)blockIdx.x * kWaves + (tid >> 6)] = nbad;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * range;
    for (uint32_t s = tid; s < range; s += kTPB) {
        out.cnt[base + s] = s_cnt[s];
        out.sum[base + s] = (long long)s_sum[s];
        out.mn[base + s] = s_mn[s];
        out.mx[base + s] = s_mx[s];
    }
}

// The matching rows' number and every key column's min and max over them (the identity for a
// column that is not there).
struct ByBounds {
    u64 count;
    int mn[kMaxKeys];
    int mx[kMaxKeys];
};

// One pass over the predicates and the surviving lines of all NK key columns: one ByBounds a
// block, combined by k_group_by_where_bounds_fold.
template <int NK, bool VEC>
__global__ __launch_bounds__(kTPB, 8) void k_group_by_where_bounds(WhereArgs w, ByArgs a, uint64_t n, uint64_t rows_per_block,
                                                                   ByBounds* __restrict__ part) {
    constexpr int U = bw_tiles(NK);
    __shared__ ByBounds sp[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;

    uint32_t cnt = 0;
    int mn[NK], mx[NK];
#pragma unroll
    for (int j = 0; j < NK; j++) {
        mn[j] = INT_MAX;
        mx[j] = INT_MIN;
    }
    auto fold = [&](int j, int4 k, uint32_t live) {
        mn[j] = min(mn[j], min(min(live & 1u ? k.x : INT_MAX, live & 2u ? k.y : INT_MAX),
                               min(live & 4u ? k.z : INT_MAX, live & 8u ? k.w : INT_MAX)));
        mx[j] = max(mx[j], max(max(live & 1u ? k.x : INT_MIN, live & 2u ? k.y : INT_MIN),
                               max(live & 4u ? k.z : INT_MIN, live & 8u ? k.w : INT_MIN)));
    };
    auto tiles = [&](auto tc, uint64_t t) {
        constexpr int T = decltype(tc)::value;
        const uint64_t row = t + (uint64_t)tid * 4;
        uint32_t live[T];
        live_tiles<VEC, T>(w, row, lane, live);
        u64 b[T];
        int4 k[T][NK];
#pragma unroll
        for (int u = 0; u < T; u++) b[u] = __ballot(live[u] != 0u);
#pragma unroll
        for (int j = 0; j < NK; j++)
#pragma unroll
            for (int u = 0; u < T; u++)
                if (b[u] != 0 && line_live(b[u], lane)) k[u][j] = load4_nt<VEC>(a.keys[j] + row + (uint64_t)u * kTileRows);
#pragma unroll
        for (int u = 0; u < T; u++)
            if (live[u] != 0u) {
                cnt += (uint32_t)__popc(live[u]);
#pragma unroll
                for (int j = 0; j < NK; j++) fold(j, k[u][j], live[u]);
            }
    };

    uint64_t t = start;
    for (; t + (uint64_t)U * kTileRows <= end; t += (uint64_t)U * kTileRows) tiles(std::integral_constant<int, U>{}, t);
    for (; t + kTileRows <= end; t += kTileRows) tiles(std::integral_constant<int, 1>{}, t);
    if (t < end) {  // the column's ragged tile
        const uint64_t row = t + (uint64_t)tid * 4;
        const uint32_t live = live_ragged(w, row, end);
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (live & (1u << e)) {
                cnt++;
#pragma unroll
                for (int j = 0; j < NK; j++) {
                    const int k = a.keys[j][row + e];
                    mn[j] = min(mn[j], k);
                    mx[j] = max(mx[j], k);
                }
            }
    }

    const u64 wc = wave_sum_u64((u64)cnt);
#pragma unroll
    for (int j = 0; j < NK; j++) {
        mn[j] = wave_min(mn[j]);
        mx[j] = wave_max(mx[j]);
    }
    if (lane == 0) {
        sp[wave].count = wc;
#pragma unroll
        for (int j = 0; j < kMaxKeys; j++) {
            sp[wave].mn[j] = INT_MAX;
            sp[wave].mx[j] = INT_MIN;
        }
#pragma unroll
        for (int j = 0; j < NK; j++) {
            sp[wave].mn[j] = mn[j];
            sp[wave].mx[j] = mx[j];
        }
    }
    __syncthreads();
    if (tid == 0) {
        ByBounds r = sp[0];
#pragma unroll
        for (int q = 1; q < kWaves; q++) {
            r.count += sp[q].count;
#pragma unroll
            for (int j = 0; j < kMaxKeys; j++) {
                r.mn[j] = min(r.mn[j], sp[q].mn[j]);
                r.mx[j] = max(r.mx[j], sp[q].mx[j]);
            }
        }
        part[blockIdx.x] = r;
    }
}

// One block: *out = the blocks' ByBounds combined.
__global__ __launch_bounds__(kTPB) void k_group_by_where_bounds_fold(const ByBounds* __restrict__ part, uint32_t blocks,
                                                                     ByBounds* __restrict__ out) {
    __shared__ ByBounds sp[kWaves];
    ByBounds r;
    r.count = 0;
#pragma unroll
    for (int j = 0; j < kMaxKeys; j++) {
        r.mn[j] = INT_MAX;
        r.mx[j] = INT_MIN;
    }
    for (uint32_t i = threadIdx.x; i < blocks; i += kTPB) {
        r.count += part[i].count;
#pragma unroll
        for (int j = 0; j < kMaxKeys; j++) {
            r.mn[j] = min(r.mn[j], part[i].mn[j]);
            r.mx[j] = max(r.mx[j], part[i].mx[j]);
        }
    }
    r.count = wave_sum_u64(r.count);
#pragma unroll
    for (int j = 0; j < kMaxKeys; j++) {
        r.mn[j] = wave_min(r.mn[j]);
        r.mx[j] = wave_max(r.mx[j]);
    }
    if ((threadIdx.x & 63) == 0) sp[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        r = sp[0];
#pragma unroll
        for (int q = 1; q < kWaves; q++) {
            r.count += sp[q].count;
#pragma unroll
            for (int j = 0; j < kMaxKeys; j++) {
                r.mn[j] = min(r.mn[j], sp[q].mn[j]);
                r.mx[j] = max(r.mx[j], sp[q].mx[j]);
            }
        }
        *out = r;
    }
}

// out[i] = code(row pos[i]) ^ 0x80000000 for the k matching rows, straight from the key
// columns (grid-stride, four independent rows a lane in flight); bad[block][wave] = the rows
// with a component out of bounds, as k_group_by_pack keeps them. A position outside [0, n)
// (mq_where_positions writes none) is counted, never used as an address.
template <int NK>
__global__ __launch_bounds__(kTPB) void k_group_by_pack_pos(ByArgs a, const int32_t* __restrict__ pos, uint32_t k, uint32_t n,
                                                            int32_t* __restrict__ out, uint32_t* __restrict__ bad) {
    constexpr int kRows = 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const u64 stride = (u64)gridDim.x * kTPB;
    uint32_t nbad = 0;
    for (u64 i0 = (u64)blockIdx.x * kTPB + tid; i0 < k; i0 += kRows * stride) {
        uint32_t p[kRows];
        bool have[kRows];
        int r[kRows][NK];
#pragma unroll
        for (int q = 0; q < kRows; q++) {
            const u64 i = i0 + q * stride;
            p[q] = i < k ? (uint32_t)pos[i] : ~0u;
            have[q] = p[q] < n;
        }
#pragma unroll
        for (int q = 0; q < kRows; q++)
#pragma unroll
            for (int j = 0; j < NK; j++) r[q][j] = have[q] ? a.keys[j][p[q]] : 0;
#pragma unroll
        for (int q = 0; q < kRows; q++) {
            const u64 i = i0 + q * stride;
            if (i >= k) continue;
            bool ok;
            const uint32_t c = row_code<NK>(a, r[q], &ok);
            nbad += ok && have[q] ? 0u : 1u;
            out[i] = (int)(c ^ 0x80000000u);
        }
    }
    nbad = (uint32_t)wave_sum_u64(nbad);
    if (lane == 0) bad[(size_t)blockIdx.x * kWaves + (tid >> 6)] = nbad;
}

// ---- several joined dimensions and fact-side keys in one tuple (mq_group_star_plan) ----

// Tiles of each column in flight per thread: kGjU with one term, by_tiles with more. NOT SWEPT:
// taken over from the kernels this one is made of; the resource report only
// shows that they fit 4 waves a SIMD without scratch.
constexpr int star_tiles_in_flight(int nt) { return nt == 1 ? kGjU : by_tiles(nt); }

// k_group_by_where_dense with the terms of a star query (mq_where_common.h: StarArgs) between
// the predicates and the tables. Term by term, in the order given: the tiles are balloted again
// and only the 128-byte lines of the term's column that still hold a row are requested
// (non-temporal); a key set term loads the bitmap word for live rows and live &= hit; a key map
// term loads the directory entry for live rows, live &= hit, then the attribute for hits (plain
// cached loads, so that they stay in L2 and the Infinity Cache); a plain term's value is the
// component. A component adds (comp - lo) * stride to the row's code and clears the row's
// in-bounds bit when comp - lo > rm1 (row_code's rule: every component by itself). Within one
// term all column loads of the iteration are issued, then all directory or bitmap loads, then
// all attribute loads, before the first use. After the last term the value column's surviving
// lines are loaded and consume() runs on slot = code, or kNoSlot for a row out of bounds, which
// is counted and never used as an address. The kind of a term is uniform over the grid.
template <int NT, bool VEC>
__global__ __launch_bounds__(kTPB, 4) void k_group_star_dense(WhereArgs w, StarArgs s, const int* vals, uint64_t n,
                                                              uint64_t rows_per_block, uint32_t range, DenseTabs out) {
    constexpr int U = star_tiles_in_flight(NT);
    __shared__ uint32_t s_cnt[kDenseSlots];
    __shared__ u64 s_sum[kDenseSlots];
    __shared__ int s_mn[kDenseSlots];
    __shared__ int s_mx[kDenseSlots];
    const int tid = threadIdx.x, lane = tid & 63;
    for (uint32_t q = tid; q < range; q += kTPB) {
        s_cnt[q] = 0u;
        s_sum[q] = 0ull;
        s_mn[q] = INT_MAX;
        s_mx[q] = INT_MIN;
    }
    __syncthreads();
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;

    uint32_t nbad = 0;  // joined rows only
    // the wave's run of tiles whose joined rows all share run_slot, folded per lane
    uint32_t run_slot = 0;
    bool run_open = false;  // wave-uniform
    uint32_t r_cnt = 0;
    long long r_sum = 0;
    int r_mn = INT_MAX, r_mx = INT_MIN;

    auto update = [&](uint32_t sl, int v) {
        if (sl < range) {  // kNoSlot never is
            atomicAdd(&s_cnt[sl], 1u);
            atomicAdd(&s_sum[sl], (u64)(long long)v);
            atomicMin(&s_mn[sl], v);
            atomicMax(&s_mx[sl], v);
        } else {
            nbad++;
        }
    };
    auto flush = [&]() {  // wave-uniform
        const uint32_t c = (uint32_t)wave_sum_u64(r_cnt);  // <= the rows of the block's chunk < 2^31
        const long long sm = wave_sum_i64(r_sum);
        const int mn = wave_min(r_mn), mx = wave_max(r_mx);
        if (lane == 0) {
            if (run_slot < range) {
                atomicAdd(&s_cnt[run_slot], c);
                atomicAdd(&s_sum[run_slot], (u64)sm);
                atomicMin(&s_mn[run_slot], mn);
                atomicMax(&s_mx[run_slot], mx);
            } else {
                nbad += c;
            }
        }
        run_open = false;
        r_cnt = 0;
        r_sum = 0;
        r_mn = INT_MAX;
        r_mx = INT_MIN;
    };
    // k_group_by_where_dense's consume on the slots of a full tile with a joined row in the wave
    auto consume = [&](uint4 sl, int4 v, uint32_t live, u64 b) {
        const uint32_t sf = live & 1u ? sl.x : live & 2u ? sl.y : live & 4u ? sl.z : sl.w;  // the lane's first joined slot
        const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)sf, __builtin_ctzll(b));
        const bool same = live == 0u || ((!(live & 1u) || sl.x == s0) && (!(live & 2u) || sl.y == s0) &&
                                         (!(live & 4u) || sl.z == s0) && (!(live & 8u) || sl.w == s0));
        if (__all(same)) {  // the joined rows of the wave's 256 share one slot: into the run
            if (run_open && s0 != run_slot) flush();
            run_slot = s0;
            run_open = true;
            r_cnt += (uint32_t)__popc(live);
            r_sum += (live & 1u ? (long long)v.x : 0ll) + (live & 2u ? (long long)v.y : 0ll) +
                     (live & 4u ? (long long)v.z : 0ll) + (live & 8u ? (long long)v.w : 0ll);
            r_mn = min(r_mn, min(min(live & 1u ? v.x : INT_MAX, live & 2u ? v.y : INT_MAX),
                                 min(live & 4u ? v.z : INT_MAX, live & 8u ? v.w : INT_MAX)));
            r_mx = max(r_mx, max(max(live & 1u ? v.x : INT_MIN, live & 2u ? v.y : INT_MIN),
                                 max(live & 4u ? v.z : INT_MIN, live & 8u ? v.w : INT_MIN)));
        } else {
            if (live & 1u) update(sl.x, v.x);
            if (live & 2u) update(sl.y, v.y);
            if (live & 4u) update(sl.z, v.z);
            if (live & 8u) update(sl.w, v.w);
        }
    };
    // One component of the lane's four rows into their codes and in-bounds bits.
    auto add_comp = [&](const StarTerm& tm, int4 c, uint4& code, uint32_t& in) {
        const uint32_t d0 = (uint32_t)c.x - tm.lo, d1 = (uint32_t)c.y - tm.lo, d2 = (uint32_t)c.z - tm.lo, d3 = (uint32_t)c.w - tm.lo;
        in &= (uint32_t)(d0 <= tm.rm1) | ((uint32_t)(d1 <= tm.rm1) << 1) | ((uint32_t)(d2 <= tm.rm1) << 2) |
              ((uint32_t)(d3 <= tm.rm1) << 3);
        code.x += d0 * tm.stride;
        code.y += d1 * tm.stride;
        code.z += d2 * tm.stride;
        code.w += d3 * tm.stride;
    };
    auto tiles = [&](auto tc, uint64_t t) {
        constexpr int T = decltype(tc)::value;
        const uint64_t row = t + (uint64_t)tid * 4;
        uint32_t live[T], in[T];
        uint4 code[T];
        live_tiles<VEC, T>(w, row, lane, live);
#pragma unroll
        for (int u = 0; u < T; u++) {
            in[u] = 15u;
            code[u] = make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const StarTerm& tm = s.t[j];
            int4 fk[T];
#pragma unroll
            for (int u = 0; u < T; u++) {
                const u64 b = __ballot(live[u] != 0u);
                fk[u] = make_int4(0, 0, 0, 0);
                if (b != 0 && line_live(b, lane)) fk[u] = load4_nt<VEC>(tm.col + row + (uint64_t)u * kTileRows);
            }
            if (tm.kind == kStarSet) {  // grid-uniform
                uint32_t bw[T][4];
#pragma unroll
                for (int u = 0; u < T; u++) {
                    bw[u][0] = live[u] & 1u ? star_word(tm, (uint32_t)fk[u].x - tm.klo) : 0u;
                    bw[u][1] = live[u] & 2u ? star_word(tm, (uint32_t)fk[u].y - tm.klo) : 0u;
                    bw[u][2] = live[u] & 4u ? star_word(tm, (uint32_t)fk[u].z - tm.klo) : 0u;
                    bw[u][3] = live[u] & 8u ? star_word(tm, (uint32_t)fk[u].w - tm.klo) : 0u;
                }
#pragma unroll
                for (int u = 0; u < T; u++)
                    live[u] &= ((bw[u][0] >> (((uint32_t)fk[u].x - tm.klo) & 31u)) & 1u) |
                               (((bw[u][1] >> (((uint32_t)fk[u].y - tm.klo) & 31u)) & 1u) << 1) |
                               (((bw[u][2] >> (((uint32_t)fk[u].z - tm.klo) & 31u)) & 1u) << 2) |
                               (((bw[u][3] >> (((uint32_t)fk[u].w - tm.klo) & 31u)) & 1u) << 3);
            } else if (tm.kind == kStarMap) {
                const MapArgs m = star_map(tm);
                u64 e[T][4];
                int4 at[T];
#pragma unroll
                for (int u = 0; u < T; u++) {  // the directory entries of the surviving rows
                    e[u][0] = live[u] & 1u ? map_entry(m, (uint32_t)fk[u].x - m.lo) : 0ull;
                    e[u][1] = live[u] & 2u ? map_entry(m, (uint32_t)fk[u].y - m.lo) : 0ull;
                    e[u][2] = live[u] & 4u ? map_entry(m, (uint32_t)fk[u].z - m.lo) : 0ull;
                    e[u][3] = live[u] & 8u ? map_entry(m, (uint32_t)fk[u].w - m.lo) : 0ull;
                }
#pragma unroll
                for (int u = 0; u < T; u++) {  // live &= hit; the attributes of the rows still joined
                    const uint32_t d0 = (uint32_t)fk[u].x - m.lo, d1 = (uint32_t)fk[u].y - m.lo, d2 = (uint32_t)fk[u].z - m.lo,
                                   d3 = (uint32_t)fk[u].w - m.lo;
                    live[u] &= (uint32_t)map_hit(e[u][0], d0) | ((uint32_t)map_hit(e[u][1], d1) << 1) |
                               ((uint32_t)map_hit(e[u][2], d2) << 2) | ((uint32_t)map_hit(e[u][3], d3) << 3);
                    at[u] = make_int4((int)tm.lo, (int)tm.lo, (int)tm.lo, (int)tm.lo);  // of a dropped row: in bounds, never used
                    if (live[u] & 1u) at[u].x = m.attr[map_rank(e[u][0], d0)];
                    if (live[u] & 2u) at[u].y = m.attr[map_rank(e[u][1], d1)];
                    if (live[u] & 4u) at[u].z = m.attr[map_rank(e[u][2], d2)];
                    if (live[u] & 8u) at[u].w = m.attr[map_rank(e[u][3], d3)];
                }
#pragma unroll
                for (int u = 0; u < T; u++) add_comp(tm, at[u], code[u], in[u]);
            } else {
#pragma unroll
                for (int u = 0; u < T; u++) add_comp(tm, fk[u], code[u], in[u]);  // of a dead row: never read below
            }
        }
        u64 b[T];
        int4 v[T];
#pragma unroll
        for (int u = 0; u < T; u++) {
            b[u] = __ballot(live[u] != 0u);
            if (b[u] != 0 && line_live(b[u], lane)) v[u] = load4_nt<VEC>(vals + row + (uint64_t)u * kTileRows);
        }
#pragma unroll
        for (int u = 0; u < T; u++)
            if (b[u] != 0)  // wave-uniform
                consume(make_uint4(in[u] & 1u ? code[u].x : kNoSlot, in[u] & 2u ? code[u].y : kNoSlot, in[u] & 4u ? code[u].z : kNoSlot,
                                   in[u] & 8u ? code[u].w : kNoSlot),
                        v[u], live[u], b[u]);
    };

    uint64_t t = start;
    for (; t + (uint64_t)U * kTileRows <= end; t += (uint64_t)U * kTileRows) tiles(std::integral_constant<int, U>{}, t);
    for (; t + kTileRows <= end; t += kTileRows) tiles(std::integral_constant<int, 1>{}, t);
    if (t < end) {  // the column's ragged tile: row by row, none past the end
        const uint64_t row = t + (uint64_t)tid * 4;
        const uint32_t live = live_ragged(w, row, end);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (!(live & (1u << i))) continue;
            uint32_t code = 0;
            bool joined = true, ok = true;
#pragma unroll
            for (int j = 0; j < NT; j++) {
                if (!joined) continue;
                const StarTerm& tm = s.t[j];
                int comp = tm.col[row + i];
                if (tm.kind == kStarSet) {
                    const uint32_t d = (uint32_t)comp - tm.klo;
                    joined = (star_word(tm, d) >> (d & 31u)) & 1u;
                    continue;
                }
                if (tm.kind == kStarMap) {
                    const MapArgs m = star_map(tm);
                    const uint32_t d = (uint32_t)comp - m.lo;
                    const u64 en = map_entry(m, d);
                    joined = map_hit(en, d);
                    if (!joined) continue;
                    comp = m.attr[map_rank(en, d)];
                }
                const uint32_t d = (uint32_t)comp - tm.lo;
                ok = ok && d <= tm.rm1;
                code += d * tm.stride;
            }
            if (joined) update(ok ? code : kNoSlot, vals[row + i]);
        }
    }
    if (run_open) flush();
    nbad = (uint32_t)wave_sum_u64(nbad);
    if (lane == 0) out.bad[(size_t)blockIdx.x * kWaves + (tid >> 6)] = nbad;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * range;
    for (uint32_t q = tid; q < range; q += kTPB) {
        out.cnt[base + q] = s_cnt[q];
        out.sum[base + q] = (long long)s_sum[q];
        out.mn[base + q] = s_mn[q];
        out.mx[base + q] = s_mx[q];
    }
}

// out[i] = code(row pos[i]) + add for the k joined rows of mq_star_positions (k_group_by_pack_pos'
// shape: grid-stride, four independent rows a lane in flight): every component read through the
// positions, where every lookup is a hit. add: 0x80000000 (the sorted column of a tuple, code ^
// 0x80000000) or, with one component, its lo (the component itself). bad[block][wave] = the rows
// with a component out of bounds, a lookup that missed or a position outside [0, n)
// (mq_star_positions writes neither): counted, never used as an address.
template <int NT>
__global__ __launch_bounds__(kTPB) void k_group_star_pack_pos(StarArgs s, const int32_t* __restrict__ pos, uint32_t k, uint32_t n,
                                                              uint32_t add, int32_t* __restrict__ out, uint32_t* __restrict__ bad) {
    constexpr int kRows = 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const u64 stride = (u64)gridDim.x * kTPB;
    uint32_t nbad = 0;
    for (u64 i0 = (u64)blockIdx.x * kTPB + tid; i0 < k; i0 += kRows * stride) {
        uint32_t p[kRows], code[kRows];
        bool ok[kRows];
#pragma unroll
        for (int q = 0; q < kRows; q++) {
            const u64 i = i0 + q * stride;
            p[q] = i < k ? (uint32_t)pos[i] : ~0u;
            ok[q] = p[q] < n;
            code[q] = 0;
        }
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const StarTerm& tm = s.t[j];
            if (tm.kind == kStarSet) continue;  // grid-uniform: no component
            int c[kRows];
#pragma unroll
            for (int q = 0; q < kRows; q++) c[q] = ok[q] ? tm.col[p[q]] : 0;
            if (tm.kind == kStarMap) {
                const MapArgs m = star_map(tm);
                u64 e[kRows];
#pragma unroll
                for (int q = 0; q < kRows; q++) e[q] = ok[q] ? map_entry(m, (uint32_t)c[q] - m.lo) : 0ull;
#pragma unroll
                for (int q = 0; q < kRows; q++) {
                    const uint32_t d = (uint32_t)c[q] - m.lo;
                    ok[q] = ok[q] && map_hit(e[q], d);
                    c[q] = ok[q] ? m.attr[map_rank(e[q], d)] : 0;
                }
            }
#pragma unroll
            for (int q = 0; q < kRows; q++) {
                const uint32_t d = (uint32_t)c[q] - tm.lo;
                ok[q] = ok[q] && d <= tm.rm1;
                code[q] += d * tm.stride;
            }
        }
#pragma unroll
        for (int q = 0; q < kRows; q++) {
            const u64 i = i0 + q * stride;
            if (i >= k) continue;
            nbad += ok[q] ? 0u : 1u;
            out[i] = (int)(code[q] + add);
        }
    }
    nbad = (uint32_t)wave_sum_u64(nbad);
    if (lane == 0) bad[(size_t)blockIdx.x * kWaves + (tid >> 6)] = nbad;
}

// ---- the sort path ----

// ccnt[b] = run heads in block b's chunk of the sorted keys; *groups = their total.
__global__ __launch_bounds__(kTPB) void k_group_heads(const int32_t* __restrict__ sorted, uint32_t n, uint64_t chunk,
                                                      uint32_t* __restrict__ ccnt, u64* __restrict__ groups) {
    __shared__ uint32_t s_w[kWaves];
    const uint64_t i0 = (uint64_t)blockIdx.x * chunk;
    const uint64_t i1 = i0 + chunk < n ? i0 + chunk : n;
    uint32_t c = 0;
    for (uint64_t i = i0 + threadIdx.x; i < i1; i += kTPB) c += i == 0 || sorted[i] != sorted[i - 1];
    const uint32_t total = block_sum(c, s_w);
    if (threadIdx.x == 0) {
        ccnt[blockIdx.x] = total;
        if (total) atomicAdd(groups, (u64)total);
    }
}

struct GroupOut {
    int32_t* keys;
    u64* count;
    long long* sum;
    int32_t* mn;
    int32_t* mx;
    u64 groups;
};

// One block. The group open at the end of chunk b, the last of the heads in chunks 0..b,
// is the only one that rows of several chunks can belong to: it receives the identity.
__global__ __launch_bounds__(kTPB) void k_group_seg_init(const uint32_t* __restrict__ ccnt, uint32_t blocks, GroupOut o) {
    __shared__ uint32_t s_w[kWaves];
    u64 run = 0;
    for (uint32_t b0 = 0; b0 < blocks; b0 += kTPB) {  // block-uniform trip count
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t v = b < blocks ? ccnt[b] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_scan(v, s_w, &total);
        const u64 incl = run + ex + v;
        if (b < blocks && incl > 0 && incl <= o.groups) {
            const u64 g = incl - 1;
            if (o.count) o.count[g] = 0ull;
            if (o.sum) o.sum[g] = 0ll;
            if (o.mn) o.mn[g] = INT_MAX;
            if (o.mx) o.mx[g] = INT_MIN;
        }
        run += total;
    }
}

struct Run {  // one run's aggregate while it is open
    u64 cnt;
    long long sum;
    int mn, mx;
};

__device__ __forceinline__ void emit_run(const GroupOut& o, u64 g, const Run& r, bool atomic) {
    if (g >= o.groups) return;  // never: g counts heads, the plan counted the same heads
    if (atomic) {
        if (o.count) atomicAdd(o.count + g, r.cnt);
        if (o.sum) atomicAdd(reinterpret_cast<u64*>(o.sum) + g, (u64)r.sum);
        if (o.mn) atomicMin(o.mn + g, r.mn);
        if (o.mx) atomicMax(o.mx + g, r.mx);
    } else {
        if (o.count) o.count[g] = r.cnt;
        if (o.sum) o.sum[g] = r.sum;
        if (o.mn) o.mn[g] = r.mn;
        if (o.mx) o.mx[g] = r.mx;
    }
}

// Row i of the sorted keys belongs to group (heads in [0, i]) - 1. Within a tile, local
// slot l = heads in the tile up to and including the row: slot 0 continues the run open
// before the tile, slot nh (the tile's head count) is open at its end.
__global__ __launch_bounds__(kTPB) void k_group_seg_write(const int32_t* __restrict__ sorted, const u64* __restrict__ pos,
                                                          const int32_t* __restrict__ vals, uint32_t n, uint64_t chunk,
                                                          const uint32_t* __restrict__ ccnt, int need_vals, GroupOut o) {
    __shared__ uint32_t s_c[kSegTile + 1];
    __shared__ u64 s_s[kSegTile + 1];
    __shared__ int s_mn[kSegTile + 1];
    __shared__ int s_mx[kSegTile + 1];
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint32_t s_hc[kSegU][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t below = 0;
    for (uint32_t i = tid; i < blockIdx.x; i += kTPB) below += ccnt[i];
    u64 base = block_sum(below, s_w);  // heads before the tile (< 2^31)
    const uint64_t i0 = (uint64_t)blockIdx.x * chunk;
    const uint64_t i1 = i0 + chunk < n ? i0 + chunk : n;
    // thread 0 keeps the open run: its group, and whether it began before this chunk
    Run car = {0ull, 0ll, INT_MAX, INT_MIN};
    u64 car_g = 0;
    bool car_valid = false, car_left = false;
    for (uint64_t s = i0; s < i1; s += kSegTile) {  // block-uniform trip count
        for (uint32_t q = tid; q <= (uint32_t)kSegTile; q += kTPB) {
            s_c[q] = 0u;
            s_s[q] = 0ull;
            s_mn[q] = INT_MAX;
            s_mx[q] = INT_MIN;
        }
        int32_t k[kSegU], v[kSegU];
        u64 p[kSegU];
        bool ok[kSegU], h[kSegU];
#pragma unroll
        for (int u = 0; u < kSegU; u++) {
            const uint64_t i = s + (uint64_t)u * kTPB + tid;
            ok[u] = i < i1;
            k[u] = ok[u] ? sorted[i] : 0;
            h[u] = ok[u] && (i == 0 || k[u] != sorted[i - 1]);
            p[u] = ok[u] && need_vals ? pos[i] : ~0ull;
        }
#pragma unroll
        for (int u = 0; u < kSegU; u++) v[u] = p[u] < n ? vals[p[u]] : 0;
        uint32_t in_wave[kSegU];
#pragma unroll
        for (int u = 0; u < kSegU; u++) {
            const u64 m = __ballot(h[u]);
            in_wave[u] = lanes_below(m);
            if (lane == 0) s_hc[u][wave] = (uint32_t)__popcll(m);
        }
        __syncthreads();  // the slots are initialised, the head counts are in
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
            atomicAdd(&s_c[l], 1u);
            if (need_vals) {
                atomicAdd(&s_s[l], (u64)(long long)v[u]);
                atomicMin(&s_mn[l], v[u]);
                atomicMax(&s_mx[l], v[u]);
            }
            if (h[u] && o.keys && base + l - 1 < o.groups) o.keys[base + l - 1] = k[u];
        }
        __syncthreads();
        for (uint32_t q = 1 + tid; q < nh; q += kTPB)  // runs that begin and end in this tile
            emit_run(o, base + q - 1, Run{s_c[q], (long long)s_s[q], s_mn[q], s_mx[q]}, false);
        if (tid == 0) {
            if (s_c[0]) {  // rows of the run open before the tile
                if (!car_valid) {  // the chunk's first tile, whose first row is no head
                    car_valid = car_left = true;
                    car_g = base - 1;
                }
                car.cnt += s_c[0];
                car.sum += (long long)s_s[0];
                car.mn = min(car.mn, s_mn[0]);
                car.mx = max(car.mx, s_mx[0]);
            }
            if (nh) {  // a head closed it; the tile's last run is open now
                if (car_valid) emit_run(o, car_g, car, car_left);
                car = Run{s_c[nh], (long long)s_s[nh], s_mn[nh], s_mx[nh]};
                car_g = base + nh - 1;
                car_valid = true;
                car_left = false;
            }
        }
        base += nh;
        __syncthreads();  // the slots are read before the next tile resets them
    }
    if (tid == 0 && car_valid) emit_run(o, car_g, car, true);  // may go on in the next chunk
}

template <bool VK, bool VV>
int launch_dense(const DevState* s, const int32_t* keys, const int32_t* vals, uint64_t n, int32_t lo, uint32_t range,
                 void** scratch_out, DenseTabs* tabs, uint32_t* blocks_out, hipStream_t st) {
    uint32_t g;
    uint64_t rpb;
    geometry(s, n, reinterpret_cast<const void*>(&k_group_dense<VK, VV>), &g, &rpb);
    void* scratch = pool_alloc(dense_scratch_bytes(g, range));
    if (!scratch) return set_err(MQ_ENOMEM, "mq_group_plan: scratch allocation failed");
    *tabs = dense_tabs(scratch, g, range);
    *scratch_out = scratch;
    *blocks_out = g;
    hipLaunchKernelGGL((k_group_dense<VK, VV>), dim3(g), dim3(kTPB), 0, st, keys, vals, n, rpb, lo, range, *tabs);
    LAUNCHCHK("k_group_dense");
    return MQ_OK;
}

template <bool VEC>
int launch_where_dense(const DevState* s, const WhereArgs& a, const int32_t* keys, const int32_t* vals, uint64_t n,
                       int32_t lo, uint32_t range, void** scratch_out, DenseTabs* tabs, uint32_t* blocks_out,
                       hipStream_t st) {
    uint32_t g;
    uint64_t rpb;
    geometry(s, n, reinterpret_cast<const void*>(&k_group_where_dense<VEC>), &g, &rpb, (uint64_t)kGwU * kTileRows);
    void* scratch = pool_alloc(dense_scratch_bytes(g, range));
    if (!scratch) return set_err(MQ_ENOMEM, "mq_group_where_plan: scratch allocation failed");
    *tabs = dense_tabs(scratch, g, range);
    *scratch_out = scratch;
    *blocks_out = g;
    hipLaunchKernelGGL((k_group_where_dense<VEC>), dim3(g), dim3(kTPB), 0, st, a, keys, vals, n, rpb, lo, range, *tabs);
    LAUNCHCHK("k_group_where_dense");
    return MQ_OK;
}

template <bool VEC>
int launch_join_dense(const DevState* s, const WhereArgs& a, const MapArgs& m, const int32_t* vals, uint64_t n, int32_t lo,
                      uint32_t range, void** scratch_out, DenseTabs* tabs, uint32_t* blocks_out, hipStream_t st) {
    uint32_t g;
    uint64_t rpb;
    geometry(s, n, reinterpret_cast<const void*>(&k_group_join_dense<VEC>), &g, &rpb, (uint64_t)kGjU * kTileRows);
    void* scratch = pool_alloc(dense_scratch_bytes(g, range));
    if (!scratch) return set_err(MQ_ENOMEM, "mq_group_join_plan: scratch allocation failed");
    *tabs = dense_tabs(scratch, g, range);
    *scratch_out = scratch;
    *blocks_out = g;
    hipLaunchKernelGGL((k_group_join_dense<VEC>), dim3(g), dim3(kTPB), 0, st, a, m, vals, n, rpb, lo, range, *tabs);
    LAUNCHCHK("k_group_join_dense");
    return MQ_OK;
}

template <int NK, bool VEC>
int launch_by_dense(const DevState* s, const ByArgs& a, const int32_t* vals, uint64_t n, uint32_t range, void** scratch_out,
                    DenseTabs* tabs, uint32_t* blocks_out, hipStream_t st) {
    uint32_t g;
    uint64_t rpb;
    geometry(s, n, reinterpret_cast<const void*>(&k_group_by_dense<NK, VEC>), &g, &rpb);
    void* scratch = pool_alloc(dense_scratch_bytes(g, range));
    if (!scratch) return set_err(MQ_ENOMEM, "mq_group_by_plan: scratch allocation failed");
    *tabs = dense_tabs(scratch, g, range);
    *scratch_out = scratch;
    *blocks_out = g;
    hipLaunchKernelGGL((k_group_by_dense<NK, VEC>), dim3(g), dim3(kTPB), 0, st, a, vals, n, rpb, range, *tabs);
    LAUNCHCHK("k_group_by_dense");
    return MQ_OK;
}

template <int NK, bool VEC>
int launch_by_where_dense(const DevState* s, const WhereArgs& w, const ByArgs& a, const int32_t* vals, uint64_t n, uint32_t range,
                          void** scratch_out, DenseTabs* tabs, uint32_t* blocks_out, hipStream_t st) {
    uint32_t g;
    uint64_t rpb;
    geometry(s, n, reinterpret_cast<const void*>(&k_group_by_where_dense<NK, VEC>), &g, &rpb, (uint64_t)bw_tiles(NK) * kTileRows);
    void* scratch = pool_alloc(dense_scratch_bytes(g, range));
    if (!scratch) return set_err(MQ_ENOMEM, "mq_group_by_where_plan: scratch allocation failed");
    *tabs = dense_tabs(scratch, g, range);
    *scratch_out = scratch;
    *blocks_out = g;
    hipLaunchKernelGGL((k_group_by_where_dense<NK, VEC>), dim3(g), dim3(kTPB), 0, st, w, a, vals, n, rpb, range, *tabs);
    LAUNCHCHK("k_group_by_where_dense");
    return MQ_OK;
}

template <int NT, bool VEC>
int launch_star_dense(const DevState* s, const WhereArgs& w, const StarArgs& a, const int32_t* vals, uint64_t n, uint32_t range,
                      void** scratch_out, DenseTabs* tabs, uint32_t* blocks_out, hipStream_t st) {
    uint32_t g;
    uint64_t rpb;
    geometry(s, n, reinterpret_cast<const void*>(&k_group_star_dense<NT, VEC>), &g, &rpb, (uint64_t)star_tiles_in_flight(NT) * kTileRows);
    void* scratch = pool_alloc(dense_scratch_bytes(g, range));
    if (!scratch) return set_err(MQ_ENOMEM, "mq_group_star_plan: scratch allocation failed");
    *tabs = dense_tabs(scratch, g, range);
    *scratch_out = scratch;
    *blocks_out = g;
    hipLaunchKernelGGL((k_group_star_dense<NT, VEC>), dim3(g), dim3(kTPB), 0, st, w, a, vals, n, rpb, range, *tabs);
    LAUNCHCHK("k_group_star_dense");
    return MQ_OK;
}

// The dense path of the plans; w: the folded predicates of mq_group_where_plan and
// mq_group_by_where_plan (wvec: whether their columns are all 16-byte aligned), or NULL; rows:
// NULL, or where the sum of the groups' counts goes; by: the nkeys key columns of
// mq_group_by_plan and mq_group_by_where_plan (keys is not used then), or NULL; jm: the key map
// of mq_group_join_plan (with w; keys is its foreign key column), or NULL; star: the terms of
// mq_group_star_plan (with w; keys is not used; the table is addressed by the tuple's code, and
// with one component by component - lo, which is that code), or NULL.
int plan_dense(const DevState* s, mq_group* g, const int32_t* keys, const int32_t* vals, uint64_t n, hipStream_t st,
               const WhereArgs* w = nullptr, bool wvec = false, uint64_t* rows = nullptr, const ByArgs* by = nullptr,
               int nkeys = 0, const MapArgs* jm = nullptr, const StarArgs* star = nullptr) {
    const char* who = star      ? "mq_group_star_plan"
                      : jm      ? "mq_group_join_plan"
                      : by && w ? "mq_group_by_where_plan"
                      : by      ? "mq_group_by_plan"
                      : w       ? "mq_group_where_plan"
                                : "mq_group_plan";
    g->tab = static_cast<char*>(pool_alloc(final_bytes(g->range)));
    if (!g->tab) return set_err(MQ_ENOMEM, "%s: table allocation failed", who);
    const FinalTab f = final_tab(g->tab, g->range);
    void* scratch = nullptr;
    DenseTabs tabs;
    uint32_t blocks = 0;
    const bool vk = aligned16(keys), vv = aligned16(vals);
    int rc;
    if (star) {
        bool vec = vv && wvec;
        for (int j = 0; j < star->nterms; j++) vec = vec && aligned16(star->t[j].col);
        auto launch = [&](auto nt) {
            constexpr int NT = decltype(nt)::value;
            return vec ? launch_star_dense<NT, true>(s, *w, *star, vals, n, g->range, &scratch, &tabs, &blocks, st)
                       : launch_star_dense<NT, false>(s, *w, *star, vals, n, g->range, &scratch, &tabs, &blocks, st);
        };
        rc = star->nterms == 1   ? launch(std::integral_constant<int, 1>{})
             : star->nterms == 2 ? launch(std::integral_constant<int, 2>{})
             : star->nterms == 3 ? launch(std::integral_constant<int, 3>{})
                                 : launch(std::integral_constant<int, 4>{});
    } else if (by) {
        bool vec = vv;
        for (int j = 0; j < nkeys; j++) vec = vec && aligned16(by->keys[j]);
        auto launch = [&](auto nk) {
            constexpr int NK = decltype(nk)::value;
            if (w)
                return vec && wvec ? launch_by_where_dense<NK, true>(s, *w, *by, vals, n, g->range, &scratch, &tabs, &blocks, st)
                                   : launch_by_where_dense<NK, false>(s, *w, *by, vals, n, g->range, &scratch, &tabs, &blocks, st);
            return vec ? launch_by_dense<NK, true>(s, *by, vals, n, g->range, &scratch, &tabs, &blocks, st)
                       : launch_by_dense<NK, false>(s, *by, vals, n, g->range, &scratch, &tabs, &blocks, st);
        };
        rc = nkeys == 2   ? launch(std::integral_constant<int, 2>{})
             : nkeys == 3 ? launch(std::integral_constant<int, 3>{})
                          : launch(std::integral_constant<int, 4>{});
    } else if (jm)
        rc = wvec && vk && vv ? launch_join_dense<true>(s, *w, *jm, vals, n, g->lo, g->range, &scratch, &tabs, &blocks, st)
                              : launch_join_dense<false>(s, *w, *jm, vals, n, g->lo, g->range, &scratch, &tabs, &blocks, st);
    else if (w)
        rc = wvec && vk && vv ? launch_where_dense<true>(s, *w, keys, vals, n, g->lo, g->range, &scratch, &tabs, &blocks, st)
                              : launch_where_dense<false>(s, *w, keys, vals, n, g->lo, g->range, &scratch, &tabs, &blocks, st);
    else
        rc = vk ? (vv ? launch_dense<true, true>(s, keys, vals, n, g->lo, g->range, &scratch, &tabs, &blocks, st)
                      : launch_dense<true, false>(s, keys, vals, n, g->lo, g->range, &scratch, &tabs, &blocks, st))
                : (vv ? launch_dense<false, true>(s, keys, vals, n, g->lo, g->range, &scratch, &tabs, &blocks, st)
                      : launch_dense<false, false>(s, keys, vals, n, g->lo, g->range, &scratch, &tabs, &blocks, st));
    u64* d_rows = nullptr;
    if (!rc && rows && !(d_rows = static_cast<u64*>(pool_alloc(sizeof(u64)))))
        rc = set_err(MQ_ENOMEM, "%s: allocation failed", who);
    if (rc) {
        pool_free_on(scratch, st);
        return rc;
    }
    hipLaunchKernelGGL(k_group_fold, dim3((g->range + kFoldSlots - 1) / kFoldSlots), dim3(kTPB), 0, st, tabs, blocks,
                       g->range, f);
    hipLaunchKernelGGL(k_group_rank, dim3(1), dim3(kTPB), 0, st, f, g->range, tabs.bad, blocks * kWaves);
    if (d_rows) hipLaunchKernelGGL(k_group_rows, dim3(1), dim3(kTPB), 0, st, f, g->range, d_rows);
    const hipError_t e = hipGetLastError();
    pool_free_on(scratch, st);  // the two kernels queued above are its last readers
    u64 h[2] = {0, 0}, r = 0;
    rc = e == hipSuccess ? MQ_OK : set_err(MQ_EHIP, "launch of k_group_fold / k_group_rank failed: %s", hipGetErrorString(e));
    if (!rc && (hipMemcpyAsync(h, f.hdr, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess ||
                (d_rows && hipMemcpyAsync(&r, d_rows, sizeof r, hipMemcpyDeviceToHost, st) != hipSuccess)))
        rc = set_err(MQ_EHIP, "%s: header download failed", who);
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = set_err(MQ_EHIP, "%s: stream failed", who);
    pool_free(d_rows);
    if (rc) return rc;
    if (h[1] && star) return set_err(MQ_EINVAL, "%s: %llu joined rows with a component outside its bounds", who, h[1]);
    if (h[1] && by) return set_err(MQ_EINVAL, "%s: %llu rows with a key outside its column's bounds", who, h[1]);
    if (h[1]) return set_err(MQ_EINVAL, "%s: %llu %s outside the bounds [%d, %lld]", who, h[1], jm ? "joined attributes" : "keys", g->lo,
                             (long long)g->lo + g->range - 1);
    g->groups = h[0];
    if (rows) *rows = r;
    return MQ_OK;
}

int plan_sort(mq_group* g, const int32_t* keys, uint64_t n, const int32_t* bounds, hipStream_t st) {
    g->sorted = static_cast<int32_t*>(pool_alloc(n * 4));
    g->pos = static_cast<u64*>(pool_alloc(n * 8));
    g->ccnt = static_cast<uint32_t*>(pool_alloc(16 + (size_t)kSegBlocks * 4));  // [groups u64][pad] then the counts
    if (!g->sorted || !g->pos || !g->ccnt) return set_err(MQ_ENOMEM, "mq_group_plan: allocation failed");
    int rc = mq_index_build(keys, n, g->sorted, reinterpret_cast<uint64_t*>(g->pos), st);  // synchronises
    if (rc) return rc;
    if (bounds) {
        int32_t ends[2];
        HIPCHK(hipMemcpyAsync(&ends[0], g->sorted, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&ends[1], g->sorted + (n - 1), 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (ends[0] < bounds[0] || ends[1] > bounds[1])
            return set_err(MQ_EINVAL, "mq_group_plan: keys [%d, %d] outside the bounds [%d, %d]", ends[0], ends[1], bounds[0],
                           bounds[1]);
    }
    seg_chunks(n, &g->blocks, &g->chunk);
    u64* hdr = reinterpret_cast<u64*>(g->ccnt);
    HIPCHK(hipMemsetAsync(hdr, 0, 16, st));
    hipLaunchKernelGGL(k_group_heads, dim3(g->blocks), dim3(kTPB), 0, st, g->sorted, (uint32_t)n, g->chunk, g->ccnt + 4, hdr);
    LAUNCHCHK("k_group_heads");
    u64 groups = 0;
    HIPCHK(hipMemcpyAsync(&groups, hdr, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    g->groups = groups;
    return MQ_OK;
}

template <int NK, bool VEC>
int launch_by_pack(const DevState* s, const ByArgs& a, uint64_t n, int32_t* packed, uint32_t** bad_out, uint32_t* nbad_out,
                   hipStream_t st) {
    uint32_t g;
    uint64_t rpb;
    geometry(s, n, reinterpret_cast<const void*>(&k_group_by_pack<NK, VEC>), &g, &rpb);
    uint32_t* bad = static_cast<uint32_t*>(pool_alloc((size_t)g * kWaves * 4));
    if (!bad) return set_err(MQ_ENOMEM, "mq_group_by_plan: allocation failed");
    *bad_out = bad;
    *nbad_out = g * kWaves;
    hipLaunchKernelGGL((k_group_by_pack<NK, VEC>), dim3(g), dim3(kTPB), 0, st, a, n, rpb, packed, bad);
    LAUNCHCHK("k_group_by_pack");
    return MQ_OK;
}

template <int NK>
int launch_by_pack_pos(const DevState* s, const ByArgs& a, const int32_t* pos, uint64_t k, uint64_t n, int32_t* packed,
                       uint32_t** bad_out, uint32_t* nbad_out, hipStream_t st) {
    const uint32_t g = stream_grid(s, (k + 3) / 4);  // four rows a lane in flight
    uint32_t* bad = static_cast<uint32_t*>(pool_alloc((size_t)g * kWaves * 4));
    if (!bad) return set_err(MQ_ENOMEM, "mq_group_by_where_plan: allocation failed");
    *bad_out = bad;
    *nbad_out = g * kWaves;
    hipLaunchKernelGGL((k_group_by_pack_pos<NK>), dim3(g), dim3(kTPB), 0, st, a, pos, (uint32_t)k, (uint32_t)n, packed, bad);
    LAUNCHCHK("k_group_by_pack_pos");
    return MQ_OK;
}

// The packed sort path: the tuples' codes as one int32 column (freed once it is sorted),
// the rows out of bounds counted on the way, then plan_sort on it. pos: NULL (all n rows), or
// the k matching rows' positions of mq_group_by_where_plan (k > 0), whose codes alone are packed.
int plan_by_sort(const DevState* s, mq_group* g, const ByArgs& a, int nkeys, uint64_t n, hipStream_t st,
                 const char* who = "mq_group_by_plan", const int32_t* pos = nullptr, uint64_t k = 0) {
    const uint64_t rows = pos ? k : n;
    int32_t* packed = static_cast<int32_t*>(pool_alloc(rows * 4));
    u64* d_total = static_cast<u64*>(pool_alloc(sizeof(u64)));
    uint32_t* bad = nullptr;
    uint32_t nbad = 0;
    int rc = packed && d_total ? MQ_OK : set_err(MQ_ENOMEM, "%s: allocation failed", who);
    if (!rc) {
        bool vec = true;
        for (int j = 0; j < nkeys; j++) vec = vec && aligned16(a.keys[j]);
        auto launch = [&](auto nk) {
            constexpr int NK = decltype(nk)::value;
            if (pos) return launch_by_pack_pos<NK>(s, a, pos, k, n, packed, &bad, &nbad, st);
            return vec ? launch_by_pack<NK, true>(s, a, n, packed, &bad, &nbad, st)
                       : launch_by_pack<NK, false>(s, a, n, packed, &bad, &nbad, st);
        };
        rc = nkeys == 2   ? launch(std::integral_constant<int, 2>{})
             : nkeys == 3 ? launch(std::integral_constant<int, 3>{})
                          : launch(std::integral_constant<int, 4>{});
    }
    u64 total = 0;
    if (!rc) {
        hipLaunchKernelGGL(k_group_by_bad, dim3(1), dim3(kTPB), 0, st, bad, nbad, d_total);
        if (hipGetLastError() != hipSuccess) rc = set_err(MQ_EHIP, "launch of k_group_by_bad failed");
    }
    if (!rc && hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, st) != hipSuccess)
        rc = set_err(MQ_EHIP, "%s: count download failed", who);
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = set_err(MQ_EHIP, "%s: stream failed", who);
    pool_free(bad);
    pool_free(d_total);
    if (!rc && total) rc = set_err(MQ_EINVAL, "%s: %llu rows with a key outside its column's bounds", who, total);
    if (!rc) rc = plan_sort(g, packed, rows, nullptr, st);  // synchronises
    pool_free_on(packed, st);
    return rc;
}

// The tuple code of the bounds b (nkeys {lo, hi} pairs whose key space is at most 2^32) over
// the key columns d_keys, as the kernels take it and as the handle keeps it for the write.
ByArgs by_args(mq_group* g, const int32_t* const* d_keys, const int32_t* b, int nkeys) {
    ByArgs a = {};
    uint64_t stride = 1;  // up to the key space
    for (int j = nkeys - 1; j >= 0; j--) {
        a.keys[j] = d_keys[j];
        a.lo[j] = (uint32_t)b[2 * j];
        a.rm1[j] = (uint32_t)((int64_t)b[2 * j + 1] - (int64_t)b[2 * j]);
        a.stride[j] = (uint32_t)stride;
        g->klo[j] = b[2 * j];
        g->krm1[j] = a.rm1[j];
        g->kstride[j] = a.stride[j];
        stride *= (uint64_t)a.rm1[j] + 1;
    }
    return a;
}

// *space = prod(hi_j - lo_j + 1) over the nkeys {lo, hi} pairs of b, saturated at 2^63;
// false: a lo > hi.
bool by_space(const int32_t* b, int nkeys, uint64_t* space) {
    uint64_t p = 1;
    for (int j = 0; j < nkeys; j++) {
        if (b[2 * j] > b[2 * j + 1]) return false;
        const uint64_t r = (uint64_t)((int64_t)b[2 * j + 1] - (int64_t)b[2 * j] + 1);  // up to 2^32
        p = p > (1ull << 63) / r ? 1ull << 63 : p * r;
    }
    *space = p;
    return true;
}

// k_group_by_where_bounds and its fold over 1..4 key columns: *found = the matching rows' number and
// every key column's min and max over them. Synchronises.
int where_key_bounds(const DevState* s, const WhereArgs& w, bool vec, const int32_t* const* d_keys, int nkeys, uint64_t n,
                     ByBounds* found, hipStream_t st, const char* who) {
    ByArgs ka = {};
    for (int j = 0; j < nkeys; j++) ka.keys[j] = d_keys[j];
    uint32_t grid = 0;
    ByBounds* part = nullptr;
    auto launch = [&](auto nk) {
        constexpr int NK = decltype(nk)::value;
        const void* fn = vec ? reinterpret_cast<const void*>(&k_group_by_where_bounds<NK, true>)
                             : reinterpret_cast<const void*>(&k_group_by_where_bounds<NK, false>);
        uint64_t rpb;
        geometry(s, n, fn, &grid, &rpb, (uint64_t)bw_tiles(NK) * kTileRows);
        part = static_cast<ByBounds*>(pool_alloc(((size_t)grid + 1) * sizeof(ByBounds)));  // the blocks', then the result
        if (!part) return set_err(MQ_ENOMEM, "%s: workspace allocation failed", who);
        if (vec)
            hipLaunchKernelGGL((k_group_by_where_bounds<NK, true>), dim3(grid), dim3(kTPB), 0, st, w, ka, n, rpb, part);
        else
            hipLaunchKernelGGL((k_group_by_where_bounds<NK, false>), dim3(grid), dim3(kTPB), 0, st, w, ka, n, rpb, part);
        LAUNCHCHK("k_group_by_where_bounds");
        return (int)MQ_OK;
    };
    int rc = nkeys == 1   ? launch(std::integral_constant<int, 1>{})
             : nkeys == 2 ? launch(std::integral_constant<int, 2>{})
             : nkeys == 3 ? launch(std::integral_constant<int, 3>{})
                          : launch(std::integral_constant<int, 4>{});
    if (!rc) {
        hipLaunchKernelGGL(k_group_by_where_bounds_fold, dim3(1), dim3(kTPB), 0, st, part, grid, part + grid);
        if (hipGetLastError() != hipSuccess) rc = set_err(MQ_EHIP, "launch of k_group_by_where_bounds_fold failed");
    }
    if (!rc && hipMemcpyAsync(found, part + grid, sizeof *found, hipMemcpyDeviceToHost, st) != hipSuccess)
        rc = set_err(MQ_EHIP, "%s: bounds download failed", who);
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = set_err(MQ_EHIP, "%s: stream failed", who);
    pool_free(part);
    return rc;
}

// The write of mq_group_write and mq_group_by_write: keys_out receives the key (one key
// column), the slot (dense, nkeys > 1) or the sorted code (sort, nkeys > 1) of every group.
int write_groups(mq_group* g, int32_t* keys_out, uint64_t* d_count_out, int64_t* d_sum_out, int32_t* d_min_out,
                 int32_t* d_max_out, hipStream_t st) {
    u64* cnt = reinterpret_cast<u64*>(d_count_out);
    long long* sum = reinterpret_cast<long long*>(d_sum_out);
    if (g->path == MQ_GROUP_DENSE) {
        hipLaunchKernelGGL(k_group_dense_write, dim3((g->range + kTPB - 1) / kTPB), dim3(kTPB), 0, st,
                           final_tab(g->tab, g->range), g->range, g->lo, keys_out, cnt, sum, d_min_out, d_max_out);
        LAUNCHCHK("k_group_dense_write");
        return MQ_OK;
    }
    const GroupOut o = {keys_out, cnt, sum, d_min_out, d_max_out, g->groups};
    const int need_vals = d_sum_out || d_min_out || d_max_out;
    hipLaunchKernelGGL(k_group_seg_init, dim3(1), dim3(kTPB), 0, st, g->ccnt + 4, g->blocks, o);
    LAUNCHCHK("k_group_seg_init");
    hipLaunchKernelGGL(k_group_seg_write, dim3(g->blocks), dim3(kTPB), 0, st, g->sorted, g->pos, g->vals, (uint32_t)g->n,
                       g->chunk, g->ccnt + 4, need_vals, o);
    LAUNCHCHK("k_group_seg_write");
    return MQ_OK;
}

void release(mq_group* g, hipStream_t st) {
    pool_free_on(g->tab, st);
    pool_free_on(g->sorted, st);
    pool_free_on(g->pos, st);
    pool_free_on(g->ccnt, st);
    pool_free_on(g->own_vals, st);
    delete g;
}

}  // namespace

// What mq_measures.hip shares (mq_group_impl.h): the kernels above stay this unit's own.
namespace mqi {

bool group_key_space(const int32_t* b, int nkeys, uint64_t* space) { return by_space(b, nkeys, space); }

void group_launch_star_pack_pos(const StarArgs& a, uint32_t grid, const int32_t* pos, uint32_t k, uint32_t n, uint32_t add,
                                int32_t* packed, uint32_t* bad, hipStream_t st) {
    auto launch = [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        hipLaunchKernelGGL((k_group_star_pack_pos<NT>), dim3(grid), dim3(kTPB), 0, st, a, pos, k, n, add, packed, bad);
    };
    if (a.nterms == 1) launch(std::integral_constant<int, 1>{});
    else if (a.nterms == 2) launch(std::integral_constant<int, 2>{});
    else if (a.nterms == 3) launch(std::integral_constant<int, 3>{});
    else launch(std::integral_constant<int, 4>{});
}

int group_where_key_bounds(const DevState* s, const WhereArgs& w, bool vec, const int32_t* const* d_keys, int nkeys, uint64_t n,
                           uint64_t* rows, int32_t* bounds, hipStream_t st, const char* who) {
    ByBounds found = {};
    const int rc = where_key_bounds(s, w, vec, d_keys, nkeys, n, &found, st, who);
    if (rc) return rc;
    *rows = found.count;
    for (int j = 0; j < nkeys; j++) {
        bounds[2 * j] = found.mn[j];
        bounds[2 * j + 1] = found.mx[j];
    }
    return MQ_OK;
}

int group_launch_pack(const DevState* s, const ByArgs& a, int nkeys, uint64_t n, const int32_t* pos, uint64_t k, int32_t* packed,
                      uint32_t** bad, uint32_t* nbad, hipStream_t st) {
    bool vec = true;
    for (int j = 0; j < nkeys; j++) vec = vec && aligned16(a.keys[j]);
    auto launch = [&](auto nk) {
        constexpr int NK = decltype(nk)::value;
        if (pos) return launch_by_pack_pos<NK>(s, a, pos, k, n, packed, bad, nbad, st);
        return vec ? launch_by_pack<NK, true>(s, a, n, packed, bad, nbad, st) : launch_by_pack<NK, false>(s, a, n, packed, bad, nbad, st);
    };
    return nkeys == 1   ? launch(std::integral_constant<int, 1>{})
           : nkeys == 2 ? launch(std::integral_constant<int, 2>{})
           : nkeys == 3 ? launch(std::integral_constant<int, 3>{})
                        : launch(std::integral_constant<int, 4>{});
}

void group_launch_bad_total(const uint32_t* bad, uint32_t nbad, unsigned long long* total, hipStream_t st) {
    hipLaunchKernelGGL(k_group_by_bad, dim3(1), dim3(kTPB), 0, st, bad, nbad, total);
}

void group_launch_heads(const int32_t* sorted, uint32_t n, uint64_t chunk, uint32_t blocks, uint32_t* ccnt,
                        unsigned long long* groups, hipStream_t st) {
    hipLaunchKernelGGL(k_group_heads, dim3(blocks), dim3(kTPB), 0, st, sorted, n, chunk, ccnt, groups);
}

void group_launch_unpack(const int32_t* codes, uint64_t groups, const int32_t* klo, const uint32_t* krm1, const uint32_t* kstride,
                         int nkeys, uint32_t flip, int32_t* const* keys_out, uint32_t grid, hipStream_t st) {
    ByArgs a = {};
    ByKeysOut o = {};
    for (int j = 0; j < nkeys; j++) {
        a.lo[j] = (uint32_t)klo[j];
        a.rm1[j] = krm1[j];
        a.stride[j] = kstride[j];
        o.keys[j] = keys_out[j];
    }
    hipLaunchKernelGGL(k_group_by_unpack, dim3(grid), dim3(kTPB), 0, st, codes, (u64)groups, a, nkeys, flip, o);
}

}  // namespace mqi

extern "C" {

uint32_t mq_group_dense_slots(void) { return kDenseSlots; }

void mq_group_sort_geometry(uint64_t n, uint32_t* blocks, uint64_t* chunk_rows) {
    uint32_t b;
    uint64_t c;
    seg_chunks(n, &b, &c);
    if (blocks) *blocks = b;
    if (chunk_rows) *chunk_rows = c;
}

int mq_group_plan(const int32_t* d_keys, const int32_t* d_vals, uint64_t n, const int32_t* h_key_bounds, int path,
                  mq_group** out, uint64_t* h_groups, int* h_path, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (out) *out = nullptr;
    if (h_groups) *h_groups = 0;
    if (!out || !h_groups || (n && (!d_keys || !d_vals))) return set_err(MQ_EINVAL, "mq_group_plan: NULL pointer");
    if (path != MQ_GROUP_AUTO && path != MQ_GROUP_DENSE && path != MQ_GROUP_SORT)
        return set_err(MQ_EINVAL, "mq_group_plan: path %d", path);
    if (n >= (1ull << 31)) return set_err(MQ_EINVAL, "mq_group_plan: n >= 2^31");
    if ((reinterpret_cast<uintptr_t>(d_keys) & 3u) || (reinterpret_cast<uintptr_t>(d_vals) & 3u))
        return set_err(MQ_EINVAL, "mq_group_plan: column not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int dev = -1;
    if ((rc = current_device(&dev))) return rc;
    mq_group* g = new (std::nothrow) mq_group();
    if (!g) return set_err(MQ_ENOMEM, "mq_group_plan: out of host memory");
    g->dev = dev;
    g->n = n;
    g->vals = d_vals;
    g->stream = st;
    if (n == 0) {
        g->path = path == MQ_GROUP_SORT ? MQ_GROUP_SORT : MQ_GROUP_DENSE;
        if (h_path) *h_path = g->path;
        *out = g;
        return MQ_OK;
    }
    int32_t lo, hi;
    if (h_key_bounds) {
        lo = h_key_bounds[0];
        hi = h_key_bounds[1];
        if (lo > hi) {
            delete g;
            return set_err(MQ_EINVAL, "mq_group_plan: bounds [%d, %d] are empty", lo, hi);
        }
    } else {  // one more read of the keys
        char* ws = static_cast<char*>(pool_alloc(partial_bytes() + sizeof(mq_agg)));
        if (!ws) {
            delete g;
            return set_err(MQ_ENOMEM, "mq_group_plan: workspace allocation failed");
        }
        mq_agg a = {};
        mq_agg* d_agg = reinterpret_cast<mq_agg*>(ws + partial_bytes());
        rc = mq_reduce(d_keys, n, d_agg, ws, partial_bytes(), stream);
        if (!rc && hipMemcpyAsync(&a, d_agg, sizeof a, hipMemcpyDeviceToHost, st) != hipSuccess)
            rc = set_err(MQ_EHIP, "mq_group_plan: bounds download failed");
        if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = set_err(MQ_EHIP, "mq_group_plan: stream failed");
        pool_free(ws);
        if (rc) {
            delete g;
            return rc;
        }
        lo = a.min;
        hi = a.max;
    }
    const int64_t range = (int64_t)hi - (int64_t)lo + 1;  // up to 2^32
    if (path == MQ_GROUP_DENSE && range > (int64_t)kDenseSlots) {
        delete g;
        return set_err(MQ_EINVAL, "mq_group_plan: key range %lld exceeds the dense path's %u slots", (long long)range,
                       kDenseSlots);
    }
    g->path = path != MQ_GROUP_AUTO ? path : range <= (int64_t)kDenseSlots ? MQ_GROUP_DENSE : MQ_GROUP_SORT;
    if (g->path == MQ_GROUP_DENSE) {
        g->lo = lo;
        g->range = (uint32_t)range;
        rc = plan_dense(s, g, d_keys, d_vals, n, st);
    } else {
        rc = plan_sort(g, d_keys, n, h_key_bounds, st);
    }
    if (rc) {
        release(g, st);
        return rc;
    }
    if (h_path) *h_path = g->path;
    *h_groups = g->groups;
    *out = g;
    return MQ_OK;
}

int mq_group_where_plan(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols, const int32_t* d_keys,
                        const int32_t* d_vals, uint64_t n, const int32_t* h_key_bounds, int path, mq_group** out,
                        uint64_t* h_groups, int* h_path, uint64_t* h_rows, void* stream) {
    const char* who = "mq_group_where_plan";
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (out) *out = nullptr;
    if (h_groups) *h_groups = 0;
    if (h_rows) *h_rows = 0;
    if (!out || !h_groups || !d_cols || !h_ranges) return set_err(MQ_EINVAL, "%s: NULL pointer", who);
    if (ncols < 1 || ncols > MQ_WHERE_MAX_COLS)
        return set_err(MQ_EINVAL, "%s: ncols %d outside 1..%d", who, ncols, (int)MQ_WHERE_MAX_COLS);
    if (path != MQ_GROUP_AUTO && path != MQ_GROUP_DENSE && path != MQ_GROUP_SORT)
        return set_err(MQ_EINVAL, "%s: path %d", who, path);
    if (n >= (1ull << 31)) return set_err(MQ_EINVAL, "%s: n >= 2^31", who);
    if (n) {
        for (int c = 0; c < ncols; c++)
            if (!d_cols[c] || (reinterpret_cast<uintptr_t>(d_cols[c]) & 3u))
                return set_err(MQ_EINVAL, "%s: column %d NULL or not 4-byte aligned", who, c);
        if (!d_keys || !d_vals || (reinterpret_cast<uintptr_t>(d_keys) & 3u) || (reinterpret_cast<uintptr_t>(d_vals) & 3u))
            return set_err(MQ_EINVAL, "%s: key or value column NULL or not 4-byte aligned", who);
        if (h_key_bounds && h_key_bounds[0] > h_key_bounds[1])
            return set_err(MQ_EINVAL, "%s: bounds [%d, %d] are empty", who, h_key_bounds[0], h_key_bounds[1]);
    }
    hipStream_t st = (hipStream_t)stream;
    int dev = -1;
    if ((rc = current_device(&dev))) return rc;
    WhereArgs a;
    bool empty, vec;
    fold_ranges(d_cols, h_ranges, ncols, &a, &empty, &vec);
    mq_group* g = new (std::nothrow) mq_group();
    if (!g) return set_err(MQ_ENOMEM, "%s: out of host memory", who);
    g->dev = dev;
    g->n = n;
    g->vals = d_vals;
    g->stream = st;
    g->path = path == MQ_GROUP_SORT ? MQ_GROUP_SORT : MQ_GROUP_DENSE;  // what a plan without rows reports
    auto no_groups = [&]() {
        if (h_path) *h_path = g->path;
        *out = g;
        return MQ_OK;
    };
    if (n == 0 || empty) return no_groups();

    // The workspace of mq_where_agg (the bounds) and of mq_where_positions (the sort path).
    void* ws = nullptr;
    const size_t ws_bytes = mq_where_workspace_bytes(n);
    auto fail = [&](int code) {
        pool_free_on(ws, st);
        release(g, st);
        return code;
    };
    int32_t lo, hi;
    uint64_t rows = 0;
    bool rows_known = false;
    if (h_key_bounds) {
        lo = h_key_bounds[0];
        hi = h_key_bounds[1];
    } else {  // one more pass over the predicates and the key lines that hold a survivor
        ws = pool_alloc(ws_bytes);
        mq_agg* d_agg = static_cast<mq_agg*>(pool_alloc(sizeof(mq_agg)));
        mq_agg ag = {};
        rc = ws && d_agg ? MQ_OK : set_err(MQ_ENOMEM, "%s: workspace allocation failed", who);
        if (!rc) rc = mq_where_agg(d_cols, h_ranges, ncols, d_keys, n, d_agg, ws, ws_bytes, stream);
        if (!rc && hipMemcpyAsync(&ag, d_agg, sizeof ag, hipMemcpyDeviceToHost, st) != hipSuccess)
            rc = set_err(MQ_EHIP, "%s: bounds download failed", who);
        if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = set_err(MQ_EHIP, "%s: stream failed", who);
        pool_free(d_agg);
        if (rc) return fail(rc);
        if (ag.count == 0) {
            pool_free(ws);
            return no_groups();
        }
        lo = ag.min;
        hi = ag.max;
        rows = ag.count;
        rows_known = true;
    }
    const int64_t range = (int64_t)hi - (int64_t)lo + 1;  // up to 2^32
    if (path == MQ_GROUP_DENSE && range > (int64_t)kDenseSlots)
        return fail(set_err(MQ_EINVAL, "%s: key range %lld exceeds the dense path's %u slots", who, (long long)range,
                            kDenseSlots));
    g->path = path != MQ_GROUP_AUTO ? path : range <= (int64_t)kDenseSlots ? MQ_GROUP_DENSE : MQ_GROUP_SORT;
    if (g->path == MQ_GROUP_DENSE) {
        pool_free(ws);  // idle: mq_where_agg's stream has been waited for
        ws = nullptr;
        g->lo = lo;
        g->range = (uint32_t)range;
        rc = plan_dense(s, g, d_keys, d_vals, n, st, &a, vec, rows_known || !h_rows ? nullptr : &rows);
        if (rc) return fail(rc);
    } else {
        // the K matching rows' positions, then their keys and values, then the sort path on those
        if (!ws) ws = pool_alloc(ws_bytes);
        int32_t* pos = static_cast<int32_t*>(pool_alloc(n * 4));
        u64* d_k = static_cast<u64*>(pool_alloc(sizeof(u64)));
        u64 k = 0;
        rc = ws && pos && d_k ? MQ_OK : set_err(MQ_ENOMEM, "%s: allocation failed", who);
        if (!rc)
            rc = mq_where_positions(d_cols, h_ranges, ncols, nullptr, n, pos, reinterpret_cast<uint64_t*>(d_k), ws, ws_bytes,
                                    stream);
        if (!rc && hipMemcpyAsync(&k, d_k, sizeof k, hipMemcpyDeviceToHost, st) != hipSuccess)
            rc = set_err(MQ_EHIP, "%s: count download failed", who);
        if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = set_err(MQ_EHIP, "%s: stream failed", who);
        pool_free(d_k);
        pool_free(ws);
        ws = nullptr;
        int32_t* ck = nullptr;
        if (!rc && k) {
            ck = static_cast<int32_t*>(pool_alloc(k * 4));
            g->own_vals = static_cast<int32_t*>(pool_alloc(k * 4));
            if (!ck || !g->own_vals) rc = set_err(MQ_ENOMEM, "%s: allocation failed", who);
            if (!rc) rc = mq_fetch(d_keys, pos, k, ck, stream);
            if (!rc) rc = mq_fetch(d_vals, pos, k, g->own_vals, stream);
        }
        pool_free_on(pos, st);  // the gathers queued above are its last readers
        if (!rc && k) {
            g->vals = g->own_vals;
            g->n = k;
            rc = plan_sort(g, ck, k, h_key_bounds, st);  // synchronises
        }
        pool_free_on(ck, st);
        if (rc) return fail(rc);
        rows = k;
    }
    if (h_path) *h_path = g->path;
    if (h_rows) *h_rows = rows;
    *h_groups = g->groups;
    *out = g;
    return MQ_OK;
}

int mq_group_join_plan(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols, const int32_t* d_fkey,
                       const mq_keymap* km, const int32_t* d_vals, uint64_t n, const int32_t* h_attr_bounds, int path,
                       mq_group** out, uint64_t* h_groups, int* h_path, uint64_t* h_rows, void* stream) {
    const char* who = "mq_group_join_plan";
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (out) *out = nullptr;
    if (h_groups) *h_groups = 0;
    if (h_rows) *h_rows = 0;
    if (!out || !h_groups || !km || (ncols > 0 && (!d_cols || !h_ranges))) return set_err(MQ_EINVAL, "%s: NULL pointer", who);
    if (ncols < 0 || ncols > MQ_WHERE_MAX_COLS)
        return set_err(MQ_EINVAL, "%s: ncols %d outside 0..%d", who, ncols, (int)MQ_WHERE_MAX_COLS);
    if (path != MQ_GROUP_AUTO && path != MQ_GROUP_DENSE && path != MQ_GROUP_SORT)
        return set_err(MQ_EINVAL, "%s: path %d", who, path);
    if (n >= (1ull << 31)) return set_err(MQ_EINVAL, "%s: n >= 2^31", who);
    if (n) {
        for (int c = 0; c < ncols; c++)
            if (!d_cols[c] || (reinterpret_cast<uintptr_t>(d_cols[c]) & 3u))
                return set_err(MQ_EINVAL, "%s: column %d NULL or not 4-byte aligned", who, c);
        if (!d_fkey || !d_vals || (reinterpret_cast<uintptr_t>(d_fkey) & 3u) || (reinterpret_cast<uintptr_t>(d_vals) & 3u))
            return set_err(MQ_EINVAL, "%s: key or value column NULL or not 4-byte aligned", who);
        if (h_attr_bounds && h_attr_bounds[0] > h_attr_bounds[1])
            return set_err(MQ_EINVAL, "%s: bounds [%d, %d] are empty", who, h_attr_bounds[0], h_attr_bounds[1]);
    }
    hipStream_t st = (hipStream_t)stream;
    int dev = -1;
    if ((rc = current_device(&dev))) return rc;
    if (dev != km->ks->dev) return set_err(MQ_EINVAL, "%s: the key map lives on device %d, the call runs on %d", who, km->ks->dev, dev);
    WhereArgs a;
    bool empty, vec;
    fold_ranges(d_cols, h_ranges, ncols, &a, &empty, &vec);
    mq_group* g = new (std::nothrow) mq_group();
    if (!g) return set_err(MQ_ENOMEM, "%s: out of host memory", who);
    g->dev = dev;
    g->n = n;
    g->vals = d_vals;
    g->stream = st;
    g->path = path == MQ_GROUP_SORT ? MQ_GROUP_SORT : MQ_GROUP_DENSE;  // what a plan without rows reports
    auto no_groups = [&]() {
        if (h_path) *h_path = g->path;
        *out = g;
        return MQ_OK;
    };
    if (n == 0 || empty || km->ks->lo > km->ks->hi) return no_groups();

    // the attribute range of the small dimension is known since the build: no pass over the fact table
    const int32_t lo = h_attr_bounds ? h_attr_bounds[0] : km->attr_lo, hi = h_attr_bounds ? h_attr_bounds[1] : km->attr_hi;
    const int64_t range = (int64_t)hi - (int64_t)lo + 1;  // up to 2^32
    if (path == MQ_GROUP_DENSE && range > (int64_t)kDenseSlots) {
        delete g;
        return set_err(MQ_EINVAL, "%s: attribute range %lld exceeds the dense path's %u slots", who, (long long)range, kDenseSlots);
    }
    g->path = path != MQ_GROUP_AUTO ? path : range <= (int64_t)kDenseSlots ? MQ_GROUP_DENSE : MQ_GROUP_SORT;
    uint64_t rows = 0;
    if (g->path == MQ_GROUP_DENSE) {
        const MapArgs m = {d_fkey, km->dir, km->attr, (uint32_t)km->ks->lo, (uint32_t)km->ks->hi - (uint32_t)km->ks->lo};
        g->lo = lo;
        g->range = (uint32_t)range;
        rc = plan_dense(s, g, d_fkey, d_vals, n, st, &a, vec, h_rows ? &rows : nullptr, nullptr, 0, &m);
        if (rc) {
            release(g, st);
            return rc;
        }
    } else {
        // the K joined rows' positions, their attributes and values, then the sort path on those
        const size_t ws_bytes = mq_semi_workspace_bytes(n);
        void* ws = pool_alloc(ws_bytes);
        int32_t* pos = static_cast<int32_t*>(pool_alloc(n * 4));
        u64* d_k = static_cast<u64*>(pool_alloc(sizeof(u64)));
        u64 k = 0;
        rc = ws && pos && d_k ? MQ_OK : set_err(MQ_ENOMEM, "%s: allocation failed", who);
        if (!rc)
            rc = mq_semi_positions(d_cols, h_ranges, ncols, d_fkey, km->ks, 0, MQ_SEMI_AUTO, nullptr, n, pos,
                                   reinterpret_cast<uint64_t*>(d_k), ws, ws_bytes, stream);
        if (!rc && hipMemcpyAsync(&k, d_k, sizeof k, hipMemcpyDeviceToHost, st) != hipSuccess)
            rc = set_err(MQ_EHIP, "%s: count download failed", who);
        if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = set_err(MQ_EHIP, "%s: stream failed", who);
        pool_free(d_k);
        pool_free(ws);
        int32_t* ck = nullptr;
        if (!rc && k) {
            ck = static_cast<int32_t*>(pool_alloc(k * 4));
            g->own_vals = static_cast<int32_t*>(pool_alloc(k * 4));
            if (!ck || !g->own_vals) rc = set_err(MQ_ENOMEM, "%s: allocation failed", who);
            if (!rc) rc = mq_keymap_lookup(km, d_fkey, pos, k, 0, ck, nullptr, stream);  // every one is a hit
            if (!rc) rc = mq_fetch(d_vals, pos, k, g->own_vals, stream);
        }
        pool_free_on(pos, st);  // the gathers queued above are its last readers
        if (!rc && k) {
            g->vals = g->own_vals;
            g->n = k;
            rc = plan_sort(g, ck, k, h_attr_bounds, st);  // synchronises
        }
        pool_free_on(ck, st);
        if (rc) {
            release(g, st);
            return rc;
        }
        rows = k;
    }
    if (h_path) *h_path = g->path;
    if (h_rows) *h_rows = rows;
    *h_groups = g->groups;
    *out = g;
    return MQ_OK;
}

int mq_group_star_plan(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols, const mq_star_term* h_terms, int nterms,
                       const int32_t* d_vals, uint64_t n, const int32_t* h_key_bounds, int path, mq_group** out,
                       uint64_t* h_groups, int* h_path, uint64_t* h_rows, void* stream) {
    const char* who = "mq_group_star_plan";
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (out) *out = nullptr;
    if (h_groups) *h_groups = 0;
    if (h_rows) *h_rows = 0;
    if (nterms < 1 || nterms > MQ_STAR_MAX_TERMS) return set_err(MQ_EINVAL, "%s: nterms %d outside 1..%d", who, nterms, (int)MQ_STAR_MAX_TERMS);
    if (!out || !h_groups || !h_terms || (ncols > 0 && (!d_cols || !h_ranges))) return set_err(MQ_EINVAL, "%s: NULL pointer", who);
    int nkeys = 0;
    for (int j = 0; j < nterms; j++) {
        if (h_terms[j].km && h_terms[j].ks) return set_err(MQ_EINVAL, "%s: term %d has both a key map and a key set", who, j);
        nkeys += h_terms[j].ks ? 0 : 1;
    }
    if (nkeys < 1 || nkeys > kMaxKeys) return set_err(MQ_EINVAL, "%s: %d components outside 1..%d", who, nkeys, kMaxKeys);
    if (ncols < 0 || ncols > MQ_WHERE_MAX_COLS)
        return set_err(MQ_EINVAL, "%s: ncols %d outside 0..%d", who, ncols, (int)MQ_WHERE_MAX_COLS);
    if (path != MQ_GROUP_AUTO && path != MQ_GROUP_DENSE && path != MQ_GROUP_SORT)
        return set_err(MQ_EINVAL, "%s: path %d", who, path);
    if (n >= (1ull << 31)) return set_err(MQ_EINVAL, "%s: n >= 2^31", who);
    int32_t b[2 * kMaxKeys];
    uint64_t space = 0;
    // the bounds given, checked before anything is allocated; bounds the plan finds, after it found them
    auto check_space = [&]() {
        if (!by_space(b, nkeys, &space)) return set_err(MQ_EINVAL, "%s: a component's bounds are empty", who);
        if (space > (1ull << 32))
            return set_err(MQ_EINVAL, "%s: the key space %llu (saturated at 2^63) is wider than 2^32", who, (u64)space);
        if (path == MQ_GROUP_DENSE && space > kDenseSlots)
            return set_err(MQ_EINVAL, "%s: the key space %llu exceeds the dense path's %u slots", who, (u64)space, kDenseSlots);
        return (int)MQ_OK;
    };
    if (n) {
        for (int c = 0; c < ncols; c++)
            if (!d_cols[c] || (reinterpret_cast<uintptr_t>(d_cols[c]) & 3u))
                return set_err(MQ_EINVAL, "%s: column %d NULL or not 4-byte aligned", who, c);
        for (int j = 0; j < nterms; j++)
            if (!h_terms[j].d_col || (reinterpret_cast<uintptr_t>(h_terms[j].d_col) & 3u))
                return set_err(MQ_EINVAL, "%s: term %d: column NULL or not 4-byte aligned", who, j);
        if (!d_vals || (reinterpret_cast<uintptr_t>(d_vals) & 3u)) return set_err(MQ_EINVAL, "%s: value column NULL or not 4-byte aligned", who);
        if (h_key_bounds) {
            for (int j = 0; j < 2 * nkeys; j++) b[j] = h_key_bounds[j];
            if ((rc = check_space())) return rc;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    int dev = -1;
    if ((rc = current_device(&dev))) return rc;
    bool none = false;  // an empty map or set among the terms: no row is joined
    for (int j = 0; j < nterms; j++) {
        const mq_keyset* ks = h_terms[j].km ? h_terms[j].km->ks : h_terms[j].ks;
        if (!ks) continue;
        if (dev != ks->dev)
            return set_err(MQ_EINVAL, "%s: term %d: the key %s lives on device %d, the call runs on %d", who, j,
                           h_terms[j].km ? "map" : "set", ks->dev, dev);
        none = none || ks->lo > ks->hi;
    }
    WhereArgs w;
    bool empty, wvec;
    fold_ranges(d_cols, h_ranges, ncols, &w, &empty, &wvec);
    const bool settled = n == 0 || empty || none;
    if (!settled && !h_key_bounds) {
        // a map's attributes are known since its build; a plain component costs one pass over its whole column
        int plain = 0;
        for (int j = 0; j < nterms; j++) plain += !h_terms[j].km && !h_terms[j].ks;
        mq_agg a[kMaxKeys] = {};
        if (plain) {
            char* ws = static_cast<char*>(pool_alloc(partial_bytes() + kMaxKeys * sizeof(mq_agg)));
            if (!ws) return set_err(MQ_ENOMEM, "%s: workspace allocation failed", who);
            mq_agg* d_agg = reinterpret_cast<mq_agg*>(ws + partial_bytes());
            for (int j = 0, q = 0; j < nterms && !rc; j++)
                if (!h_terms[j].km && !h_terms[j].ks) rc = mq_reduce(h_terms[j].d_col, n, d_agg + q++, ws, partial_bytes(), stream);
            if (!rc && hipMemcpyAsync(a, d_agg, plain * sizeof(mq_agg), hipMemcpyDeviceToHost, st) != hipSuccess)
                rc = set_err(MQ_EHIP, "%s: bounds download failed", who);
            if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = set_err(MQ_EHIP, "%s: stream failed", who);
            pool_free(ws);
            if (rc) return rc;
        }
        for (int j = 0, c = 0, q = 0; j < nterms; j++) {
            if (h_terms[j].ks) continue;
            b[2 * c] = h_terms[j].km ? h_terms[j].km->attr_lo : a[q].min;
            b[2 * c + 1] = h_terms[j].km ? h_terms[j].km->attr_hi : a[q].max;
            q += h_terms[j].km ? 0 : 1;
            c++;
        }
        if ((rc = check_space())) return rc;
    }
    mq_group* g = new (std::nothrow) mq_group();
    if (!g) return set_err(MQ_ENOMEM, "%s: out of host memory", who);
    g->dev = dev;
    g->n = n;
    g->vals = d_vals;
    g->stream = st;
    g->nkeys = nkeys > 1 ? nkeys : 0;  // one component: the one-key handle of mq_group_join_plan
    g->path = path == MQ_GROUP_SORT ? MQ_GROUP_SORT : MQ_GROUP_DENSE;  // what a plan without rows reports
    if (settled) {
        if (h_path) *h_path = g->path;
        *out = g;
        return MQ_OK;
    }
    auto fail = [&](int code) {
        release(g, st);
        return code;
    };
    g->path = path != MQ_GROUP_AUTO ? path : space <= kDenseSlots ? MQ_GROUP_DENSE : MQ_GROUP_SORT;
    // the terms as the kernels take them; the tuple's code as by_args lays it out, kept in the handle for the write
    StarArgs a = {};
    a.nterms = nterms;
    {
        uint64_t stride = 1;  // up to the key space
        for (int j = nterms - 1, c = nkeys - 1; j >= 0; j--) {
            StarTerm& t = a.t[j];
            const mq_keyset* ks = h_terms[j].km ? h_terms[j].km->ks : h_terms[j].ks;
            t.col = h_terms[j].d_col;
            t.kind = h_terms[j].km ? kStarMap : h_terms[j].ks ? kStarSet : kStarPlain;
            if (ks) {
                t.bits = ks->bits;
                t.klo = (uint32_t)ks->lo;
                t.kwm1 = (uint32_t)ks->hi - (uint32_t)ks->lo;
            }
            if (h_terms[j].km) {
                t.dir = h_terms[j].km->dir;
                t.attr = h_terms[j].km->attr;
            }
            if (h_terms[j].ks) continue;
            t.lo = (uint32_t)b[2 * c];
            t.rm1 = (uint32_t)((int64_t)b[2 * c + 1] - (int64_t)b[2 * c]);
            t.stride = (uint32_t)stride;
            if (nkeys > 1) {
                g->klo[c] = b[2 * c];
                g->krm1[c] = t.rm1;
                g->kstride[c] = t.stride;
            }
            stride *= (uint64_t)t.rm1 + 1;
            c--;
        }
    }
    uint64_t rows = 0;
    if (g->path == MQ_GROUP_DENSE) {
        g->lo = nkeys > 1 ? 0 : b[0];  // the table is addressed by the code; one component's code is component - lo
        g->range = (uint32_t)space;
        rc = plan_dense(s, g, nullptr, d_vals, n, st, &w, wvec, h_rows ? &rows : nullptr, nullptr, 0, nullptr, &a);
        if (rc) return fail(rc);
    } else {
        // the K joined rows' positions, their codes packed through them, their values, then the sort path
        const size_t ws_bytes = mq_semi_workspace_bytes(n);
        void* ws = pool_alloc(ws_bytes);
        int32_t* pos = static_cast<int32_t*>(pool_alloc(n * 4));
        u64* d_k = static_cast<u64*>(pool_alloc(sizeof(u64)));
        u64 k = 0;
        rc = ws && pos && d_k ? MQ_OK : set_err(MQ_ENOMEM, "%s: allocation failed", who);
        if (!rc)
            rc = mq_star_positions(d_cols, h_ranges, ncols, h_terms, nterms, nullptr, n, pos, reinterpret_cast<uint64_t*>(d_k), ws,
                                   ws_bytes, stream);
        if (!rc && hipMemcpyAsync(&k, d_k, sizeof k, hipMemcpyDeviceToHost, st) != hipSuccess)
            rc = set_err(MQ_EHIP, "%s: count download failed", who);
        if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = set_err(MQ_EHIP, "%s: stream failed", who);
        pool_free(d_k);
        pool_free(ws);
        int32_t* packed = nullptr;
        uint32_t* bad = nullptr;
        u64* d_total = nullptr;
        if (!rc && k) {
            packed = static_cast<int32_t*>(pool_alloc(k * 4));
            g->own_vals = static_cast<int32_t*>(pool_alloc(k * 4));
            d_total = static_cast<u64*>(pool_alloc(sizeof(u64)));
            const uint32_t grid = stream_grid(s, (k + 3) / 4);  // four rows a lane in flight
            bad = static_cast<uint32_t*>(pool_alloc((size_t)grid * kWaves * 4));
            if (!packed || !g->own_vals || !d_total || !bad) rc = set_err(MQ_ENOMEM, "%s: allocation failed", who);
            if (!rc) rc = mq_fetch(d_vals, pos, k, g->own_vals, stream);
            if (!rc) {
                const uint32_t add = nkeys > 1 ? 0x80000000u : (uint32_t)b[0];
                auto launch = [&](auto nt) {
                    constexpr int NT = decltype(nt)::value;
                    hipLaunchKernelGGL((k_group_star_pack_pos<NT>), dim3(grid), dim3(kTPB), 0, st, a, pos, (uint32_t)k, (uint32_t)n, add,
                                       packed, bad);
                };
                if (nterms == 1) launch(std::integral_constant<int, 1>{});
                else if (nterms == 2) launch(std::integral_constant<int, 2>{});
                else if (nterms == 3) launch(std::integral_constant<int, 3>{});
                else launch(std::integral_constant<int, 4>{});
                hipLaunchKernelGGL(k_group_by_bad, dim3(1), dim3(kTPB), 0, st, bad, grid * kWaves, d_total);
                if (hipGetLastError() != hipSuccess) rc = set_err(MQ_EHIP, "launch of k_group_star_pack_pos / k_group_by_bad failed");
            }
            u64 total = 0;
            if (!rc && hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, st) != hipSuccess)
                rc = set_err(MQ_EHIP, "%s: count download failed", who);
            if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = set_err(MQ_EHIP, "%s: stream failed", who);
            if (!rc && total) rc = set_err(MQ_EINVAL, "%s: %llu joined rows with a component outside its bounds", who, total);
        }
        pool_free(bad);
        pool_free(d_total);
        pool_free_on(pos, st);  // the gather and the pack queued above are its last readers
        if (!rc && k) {
            g->vals = g->own_vals;
            g->n = k;
            rc = plan_sort(g, packed, k, nullptr, st);  // synchronises
        }
        pool_free_on(packed, st);
        if (rc) return fail(rc);
        rows = k;
    }
    if (h_path) *h_path = g->path;
    if (h_rows) *h_rows = rows;
    *h_groups = g->groups;
    *out = g;
    return MQ_OK;
}

int mq_group_write(mq_group* g, int32_t* d_keys_out, uint64_t* d_count_out, int64_t* d_sum_out, int32_t* d_min_out,
                   int32_t* d_max_out, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!g) return set_err(MQ_EINVAL, "mq_group_write: NULL handle");
    int dev = -1;
    if ((rc = current_device(&dev))) return rc;
    if (dev != g->dev) return set_err(MQ_EINVAL, "mq_group_write: the plan was made on device %d", g->dev);
    if (g->nkeys > 1 && d_keys_out)
        return set_err(MQ_EINVAL, "mq_group_write: one column cannot hold a %d-key tuple (mq_group_by_write)", g->nkeys);
    if (g->groups == 0) return MQ_OK;
    hipStream_t st = (hipStream_t)stream;
    g->stream = st;
    return write_groups(g, d_keys_out, d_count_out, d_sum_out, d_min_out, d_max_out, st);
}

int mq_group_by_auto_path(const int32_t* h_key_bounds, int nkeys, uint64_t* h_space) {
    if (h_space) *h_space = 0;
    if (nkeys < 1 || nkeys > kMaxKeys) return set_err(MQ_EINVAL, "mq_group_by_auto_path: nkeys %d outside 1..%d", nkeys, kMaxKeys);
    if (!h_key_bounds) return set_err(MQ_EINVAL, "mq_group_by_auto_path: NULL pointer");
    uint64_t space;
    if (!by_space(h_key_bounds, nkeys, &space)) return set_err(MQ_EINVAL, "mq_group_by_auto_path: a column's bounds are empty");
    if (h_space) *h_space = space;
    if (space > (1ull << 32))
        return set_err(MQ_EINVAL, "mq_group_by_auto_path: the key space %llu is wider than 2^32", (u64)space);
    return space <= kDenseSlots ? MQ_GROUP_DENSE : MQ_GROUP_SORT;
}

int mq_group_by_plan(const int32_t* const* d_keys, int nkeys, const int32_t* d_vals, uint64_t n, const int32_t* h_key_bounds,
                     int path, mq_group** out, uint64_t* h_groups, int* h_path, void* stream) {
    const char* who = "mq_group_by_plan";
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (out) *out = nullptr;
    if (h_groups) *h_groups = 0;
    if (nkeys < 1 || nkeys > kMaxKeys) return set_err(MQ_EINVAL, "%s: nkeys %d outside 1..%d", who, nkeys, kMaxKeys);
    if (!out || !h_groups || (n && (!d_keys || !d_vals))) return set_err(MQ_EINVAL, "%s: NULL pointer", who);
    if (nkeys == 1) return mq_group_plan(d_keys ? d_keys[0] : nullptr, d_vals, n, h_key_bounds, path, out, h_groups, h_path, stream);
    if (path != MQ_GROUP_AUTO && path != MQ_GROUP_DENSE && path != MQ_GROUP_SORT)
        return set_err(MQ_EINVAL, "%s: path %d", who, path);
    if (n >= (1ull << 31)) return set_err(MQ_EINVAL, "%s: n >= 2^31", who);
    if (n) {
        for (int j = 0; j < nkeys; j++)
            if (!d_keys[j] || (reinterpret_cast<uintptr_t>(d_keys[j]) & 3u))
                return set_err(MQ_EINVAL, "%s: key column %d NULL or not 4-byte aligned", who, j);
        if (reinterpret_cast<uintptr_t>(d_vals) & 3u) return set_err(MQ_EINVAL, "%s: value column not 4-byte aligned", who);
    }
    hipStream_t st = (hipStream_t)stream;
    int dev = -1;
    if ((rc = current_device(&dev))) return rc;
    int32_t b[2 * kMaxKeys];
    uint64_t space = 0;
    if (n && h_key_bounds) {
        for (int j = 0; j < 2 * nkeys; j++) b[j] = h_key_bounds[j];
    } else if (n) {  // one more read of every key column
        char* ws = static_cast<char*>(pool_alloc(partial_bytes() + kMaxKeys * sizeof(mq_agg)));
        if (!ws) return set_err(MQ_ENOMEM, "%s: workspace allocation failed", who);
        mq_agg a[kMaxKeys] = {};
        mq_agg* d_agg = reinterpret_cast<mq_agg*>(ws + partial_bytes());
        for (int j = 0; j < nkeys && !rc; j++) rc = mq_reduce(d_keys[j], n, d_agg + j, ws, partial_bytes(), stream);
        if (!rc && hipMemcpyAsync(a, d_agg, nkeys * sizeof(mq_agg), hipMemcpyDeviceToHost, st) != hipSuccess)
            rc = set_err(MQ_EHIP, "%s: bounds download failed", who);
        if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = set_err(MQ_EHIP, "%s: stream failed", who);
        pool_free(ws);
        if (rc) return rc;
        for (int j = 0; j < nkeys; j++) {
            b[2 * j] = a[j].min;
            b[2 * j + 1] = a[j].max;
        }
    }
    if (n) {
        if (!by_space(b, nkeys, &space)) return set_err(MQ_EINVAL, "%s: a column's bounds are empty", who);
        if (space > (1ull << 32))
            return set_err(MQ_EINVAL, "%s: the key space %llu (saturated at 2^63) is wider than 2^32", who, (u64)space);
        if (path == MQ_GROUP_DENSE && space > kDenseSlots)
            return set_err(MQ_EINVAL, "%s: the key space %llu exceeds the dense path's %u slots", who, (u64)space, kDenseSlots);
    }
    mq_group* g = new (std::nothrow) mq_group();
    if (!g) return set_err(MQ_ENOMEM, "%s: out of host memory", who);
    g->dev = dev;
    g->n = n;
    g->vals = d_vals;
    g->stream = st;
    g->nkeys = nkeys;
    if (n == 0) {
        g->path = path == MQ_GROUP_SORT ? MQ_GROUP_SORT : MQ_GROUP_DENSE;
        if (h_path) *h_path = g->path;
        *out = g;
        return MQ_OK;
    }
    g->path = path != MQ_GROUP_AUTO ? path : space <= kDenseSlots ? MQ_GROUP_DENSE : MQ_GROUP_SORT;
    const ByArgs a = by_args(g, d_keys, b, nkeys);
    if (g->path == MQ_GROUP_DENSE) {
        g->lo = 0;  // the table is addressed by the code
        g->range = (uint32_t)space;
        rc = plan_dense(s, g, nullptr, d_vals, n, st, nullptr, false, nullptr, &a, nkeys);
    } else {
        rc = plan_by_sort(s, g, a, nkeys, n, st);
    }
    if (rc) {
        release(g, st);
        return rc;
    }
    if (h_path) *h_path = g->path;
    *h_groups = g->groups;
    *out = g;
    return MQ_OK;
}

int mq_group_by_where_plan(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols, const int32_t* const* d_keys,
                           int nkeys, const int32_t* d_vals, uint64_t n, const int32_t* h_key_bounds, int path, mq_group** out,
                           uint64_t* h_groups, int* h_path, uint64_t* h_rows, void* stream) {
    const char* who = "mq_group_by_where_plan";
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (out) *out = nullptr;
    if (h_groups) *h_groups = 0;
    if (h_rows) *h_rows = 0;
    if (nkeys < 1 || nkeys > kMaxKeys) return set_err(MQ_EINVAL, "%s: nkeys %d outside 1..%d", who, nkeys, kMaxKeys);
    if (!out || !h_groups || !d_cols || !h_ranges || (n && (!d_keys || !d_vals))) return set_err(MQ_EINVAL, "%s: NULL pointer", who);
    if (nkeys == 1)
        return mq_group_where_plan(d_cols, h_ranges, ncols, d_keys ? d_keys[0] : nullptr, d_vals, n, h_key_bounds, path, out,
                                   h_groups, h_path, h_rows, stream);
    if (ncols < 1 || ncols > MQ_WHERE_MAX_COLS)
        return set_err(MQ_EINVAL, "%s: ncols %d outside 1..%d", who, ncols, (int)MQ_WHERE_MAX_COLS);
    if (path != MQ_GROUP_AUTO && path != MQ_GROUP_DENSE && path != MQ_GROUP_SORT)
        return set_err(MQ_EINVAL, "%s: path %d", who, path);
    if (n >= (1ull << 31)) return set_err(MQ_EINVAL, "%s: n >= 2^31", who);
    int32_t b[2 * kMaxKeys];
    uint64_t space = 0;
    // the bounds given, checked before anything is allocated; bounds the plan finds, after it found them
    auto check_space = [&]() {
        if (!by_space(b, nkeys, &space)) return set_err(MQ_EINVAL, "%s: a column's bounds are empty", who);
        if (space > (1ull << 32))
            return set_err(MQ_EINVAL, "%s: the key space %llu (saturated at 2^63) is wider than 2^32", who, (u64)space);
        if (path == MQ_GROUP_DENSE && space > kDenseSlots)
            return set_err(MQ_EINVAL, "%s: the key space %llu exceeds the dense path's %u slots", who, (u64)space, kDenseSlots);
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
        if (h_key_bounds) {
            for (int j = 0; j < 2 * nkeys; j++) b[j] = h_key_bounds[j];
            if ((rc = check_space())) return rc;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    int dev = -1;
    if ((rc = current_device(&dev))) return rc;
    WhereArgs w;
    bool empty, wvec;
    fold_ranges(d_cols, h_ranges, ncols, &w, &empty, &wvec);
    mq_group* g = new (std::nothrow) mq_group();
    if (!g) return set_err(MQ_ENOMEM, "%s: out of host memory", who);
    g->dev = dev;
    g->n = n;
    g->vals = d_vals;
    g->stream = st;
    g->nkeys = nkeys;
    g->path = path == MQ_GROUP_SORT ? MQ_GROUP_SORT : MQ_GROUP_DENSE;  // what a plan without rows reports
    auto no_groups = [&]() {
        if (h_path) *h_path = g->path;
        *out = g;
        return MQ_OK;
    };
    if (n == 0 || empty) return no_groups();
    auto fail = [&](int code) {
        release(g, st);
        return code;
    };
    bool kvec = true;
    for (int j = 0; j < nkeys; j++) kvec = kvec && aligned16(d_keys[j]);
    uint64_t rows = 0;
    bool rows_known = false;
    if (!h_key_bounds) {  // one more pass over the predicates and the key lines that hold a survivor
        ByBounds found = {};
        rc = where_key_bounds(s, w, wvec && kvec, d_keys, nkeys, n, &found, st, who);  // synchronises
        if (rc) return fail(rc);
        if (found.count == 0) return no_groups();
        for (int j = 0; j < nkeys; j++) {
            b[2 * j] = found.mn[j];
            b[2 * j + 1] = found.mx[j];
        }
        rows = found.count;
        rows_known = true;
        if ((rc = check_space())) return fail(rc);
    }
    g->path = path != MQ_GROUP_AUTO ? path : space <= kDenseSlots ? MQ_GROUP_DENSE : MQ_GROUP_SORT;
    const ByArgs a = by_args(g, d_keys, b, nkeys);
    if (g->path == MQ_GROUP_DENSE) {
        g->lo = 0;  // the table is addressed by the code
        g->range = (uint32_t)space;
        rc = plan_dense(s, g, nullptr, d_vals, n, st, &w, wvec, rows_known || !h_rows ? nullptr : &rows, &a, nkeys);
        if (rc) return fail(rc);
    } else {
        // the K matching rows' positions, their codes packed through them, their values, then the sort path
        const size_t ws_bytes = mq_where_workspace_bytes(n);
        void* ws = pool_alloc(ws_bytes);
        int32_t* pos = static_cast<int32_t*>(pool_alloc(n * 4));
        u64* d_k = static_cast<u64*>(pool_alloc(sizeof(u64)));
        u64 k = 0;
        rc = ws && pos && d_k ? MQ_OK : set_err(MQ_ENOMEM, "%s: allocation failed", who);
        if (!rc)
            rc = mq_where_positions(d_cols, h_ranges, ncols, nullptr, n, pos, reinterpret_cast<uint64_t*>(d_k), ws, ws_bytes,
                                    stream);
        if (!rc && hipMemcpyAsync(&k, d_k, sizeof k, hipMemcpyDeviceToHost, st) != hipSuccess)
            rc = set_err(MQ_EHIP, "%s: count download failed", who);
        if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = set_err(MQ_EHIP, "%s: stream failed", who);
        pool_free(d_k);
        pool_free(ws);
        if (!rc && k) {
            g->own_vals = static_cast<int32_t*>(pool_alloc(k * 4));
            if (!g->own_vals) rc = set_err(MQ_ENOMEM, "%s: allocation failed", who);
            if (!rc) rc = mq_fetch(d_vals, pos, k, g->own_vals, stream);
            if (!rc) {
                g->vals = g->own_vals;
                g->n = k;
                rc = plan_by_sort(s, g, a, nkeys, n, st, who, pos, k);  // synchronises
            }
        }
        pool_free_on(pos, st);  // the gather and the pack queued above are its last readers
        if (rc) return fail(rc);
        rows = k;
    }
    if (h_path) *h_path = g->path;
    if (h_rows) *h_rows = rows;
    *h_groups = g->groups;
    *out = g;
    return MQ_OK;
}

int mq_group_by_write(mq_group* g, int32_t* const* d_keys_out, uint64_t* d_count_out, int64_t* d_sum_out, int32_t* d_min_out,
                      int32_t* d_max_out, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!g) return set_err(MQ_EINVAL, "mq_group_by_write: NULL handle");
    if (g->nkeys <= 1) return mq_group_write(g, d_keys_out ? d_keys_out[0] : nullptr, d_count_out, d_sum_out, d_min_out, d_max_out, stream);
    int dev = -1;
    if ((rc = current_device(&dev))) return rc;
    if (dev != g->dev) return set_err(MQ_EINVAL, "mq_group_by_write: the plan was made on device %d", g->dev);
    if (g->groups == 0) return MQ_OK;
    hipStream_t st = (hipStream_t)stream;
    g->stream = st;
    ByArgs a = {};
    ByKeysOut o = {};
    bool want = false;
    for (int j = 0; j < g->nkeys; j++) {
        a.lo[j] = (uint32_t)g->klo[j];
        a.rm1[j] = g->krm1[j];
        a.stride[j] = g->kstride[j];
        o.keys[j] = d_keys_out ? d_keys_out[j] : nullptr;
        want = want || o.keys[j];
    }
    int32_t* codes = nullptr;  // the groups' slots or sorted codes
    if (want && !(codes = static_cast<int32_t*>(pool_alloc(g->groups * 4))))
        return set_err(MQ_ENOMEM, "mq_group_by_write: allocation failed");
    rc = write_groups(g, codes, d_count_out, d_sum_out, d_min_out, d_max_out, st);
    if (!rc && codes) {
        hipLaunchKernelGGL(k_group_by_unpack, dim3(stream_grid(s, g->groups)), dim3(kTPB), 0, st, codes, (u64)g->groups, a,
                           g->nkeys, g->path == MQ_GROUP_DENSE ? 0u : 0x80000000u, o);
        if (hipGetLastError() != hipSuccess) rc = set_err(MQ_EHIP, "launch of k_group_by_unpack failed");
    }
    pool_free_on(codes, st);  // k_group_by_unpack is its last reader
    return rc;
}

// HAVING, ORDER BY an aggregate and LIMIT over the handle's groups: the handle's
// own write into pool buffers, mq_topk64 on the ordering and filter aggregates as int64 columns,
// the requested outputs gathered through its indices. The kernels are mq_topk64.hip's.
int mq_group_top(mq_group* g, const mq_group_order* o, uint64_t* h_m, int32_t* const* d_keys_out, uint64_t* d_count_out,
                 int64_t* d_sum_out, int32_t* d_min_out, int32_t* d_max_out, mq_topk64_info* h_info, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (h_info) *h_info = mq_topk64_info{};
    if (h_m) *h_m = 0;
    if (!g || !o || !h_m) return set_err(MQ_EINVAL, "mq_group_top: NULL pointer");
    if (o->order_by < MQ_AGG_KEY || o->order_by > MQ_AGG_MAX) return set_err(MQ_EINVAL, "mq_group_top: order_by %d", o->order_by);
    if (o->having_by < MQ_AGG_KEY || o->having_by > MQ_AGG_MAX) return set_err(MQ_EINVAL, "mq_group_top: having_by %d", o->having_by);
    if (o->path != MQ_TOPK_AUTO && o->path != MQ_TOPK_SELECT && o->path != MQ_TOPK_SORT)
        return set_err(MQ_EINVAL, "mq_group_top: path %d", o->path);
    int dev = -1;
    if ((rc = current_device(&dev))) return rc;
    if (dev != g->dev) return set_err(MQ_EINVAL, "mq_group_top: the plan was made on device %d", g->dev);
    if (g->groups == 0) return MQ_OK;
    hipStream_t st = (hipStream_t)stream;
    g->stream = st;
    const uint64_t G = g->groups;
    const int nkeys = g->nkeys > 1 ? g->nkeys : 1;
    const uint64_t cap = o->k < G ? o->k : G;

    struct Bufs {  // the call's pool buffers: freed once the stream has drained, on every way out
        void* p[kMaxKeys + 8];
        int used = 0;
        hipStream_t st;
        void* get(size_t bytes) {
            void* q = pool_alloc(bytes ? bytes : 16);
            if (q) p[used++] = q;
            return q;
        }
        ~Bufs() {
            if (used) (void)hipStreamSynchronize(st);
            for (int i = 0; i < used; i++) pool_free(p[i]);
        }
    } bufs;
    bufs.st = st;

    // every group's aggregates that order, filter or leave, as the handle writes them
    void* const outs[5] = {nullptr, d_count_out, d_sum_out, d_min_out, d_max_out};
    void* full[5] = {};
    bool ok = true;
    for (int a = MQ_AGG_COUNT; a <= MQ_AGG_MAX; a++)
        if (outs[a] || o->order_by == a || o->having_by == a)
            ok = ok && (full[a] = bufs.get(G * (a <= MQ_AGG_SUM ? 8 : 4)));
    int32_t* kfull[kMaxKeys] = {};
    for (int j = 0; j < nkeys; j++)
        if (d_keys_out && d_keys_out[j]) ok = ok && (kfull[j] = static_cast<int32_t*>(bufs.get(G * 4)));
    uint32_t* idx = static_cast<uint32_t*>(bufs.get(cap * 4));
    if (!ok || !idx) return set_err(MQ_ENOMEM, "mq_group_top: allocation failed");
    rc = mq_group_by_write(g, kfull, static_cast<uint64_t*>(full[MQ_AGG_COUNT]), static_cast<int64_t*>(full[MQ_AGG_SUM]),
                           static_cast<int32_t*>(full[MQ_AGG_MIN]), static_cast<int32_t*>(full[MQ_AGG_MAX]), stream);
    if (rc) return rc;
    // the ordering and the filter aggregate as int64 columns: a count (below 2^31) and a sum are
    // one already, a min or max is widened
    const uint32_t grid = stream_grid(s, G);
    int64_t* wide[5] = {};
    auto as64 = [&](int a) -> const int64_t* {
        if (a == MQ_AGG_KEY) return nullptr;
        if (a <= MQ_AGG_SUM) return static_cast<const int64_t*>(full[a]);
        if (!wide[a] && (wide[a] = static_cast<int64_t*>(bufs.get(G * 8))))
            topk64_launch_widen(static_cast<const int32_t*>(full[a]), G, wide[a], grid, st);
        return wide[a];
    };
    const int64_t* ord = as64(o->order_by);
    const int64_t* hav = as64(o->having_by);
    if ((o->order_by != MQ_AGG_KEY && !ord) || (o->having_by != MQ_AGG_KEY && !hav))
        return set_err(MQ_ENOMEM, "mq_group_top: allocation failed");
    LAUNCHCHK("k_topk64_widen");
    mq_topk64_info info;
    rc = mq_topk64(ord, hav, &o->having, G, o->k, o->descending, o->path, o->cand_cap, nullptr, idx, &info, stream);
    if (rc) return rc;
    const uint64_t m = info.m;
    if (m) {
        const uint32_t gm = stream_grid(s, m);
        for (int j = 0; j < nkeys; j++)
            if (kfull[j]) topk64_launch_take32(kfull[j], idx, m, d_keys_out[j], gm, st);
        for (int a = MQ_AGG_COUNT; a <= MQ_AGG_MAX; a++) {
            if (!outs[a]) continue;
            if (a <= MQ_AGG_SUM) topk64_launch_take64(static_cast<const int64_t*>(full[a]), idx, m, static_cast<int64_t*>(outs[a]), gm, st);
            else topk64_launch_take32(static_cast<const int32_t*>(full[a]), idx, m, static_cast<int32_t*>(outs[a]), gm, st);
        }
        LAUNCHCHK("k_topk64_take");
    }
    HIPCHK(hipStreamSynchronize(st));
    if (h_info) *h_info = info;
    *h_m = m;
    return MQ_OK;
}

int mq_group_free(mq_group* g) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!g) return MQ_OK;
    release(g, g->stream);  // a queued write may still read the buffers: freed in its stream's order
    return MQ_OK;
}

}  // extern "C"
