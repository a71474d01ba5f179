// mq_measures.hip — several expression aggregates over the joined rows of a star query, in one
// pass: mq_group_star_plan's rows and groups, and per group one count and, per
// measure, the sum (modulo 2^64), min and max of an int64 value computed exactly from one or two
// int32 columns: a, a + b, a - b or a * b. Every accumulation of a sum is unsigned 64-bit; min and
// max are signed 64-bit compares; so the result does not depend on the order in which blocks,
// waves or lanes contribute, and no signed overflow is ever evaluated.
//
// dense (P <= mq_group_measures_dense_slots(nmeas)):
//   k_group_measures_dense<NT, NM, VEC>: k_group_star_dense's front half (predicates, terms in
//                        order, the code and the in-bounds bits); then of the DISTINCT operand
//                        columns (the host's list, at most 2 * NM) the 128-byte lines that still
//                        hold a joined row, each column once per tile; the measures pick their
//                        operands from those registers by a grid-uniform index and op. The block's
//                        LDS table is a u32 count and, per measure, u64 sum, i64 min and i64 max
//                        per slot, updated with ds_add_u32 / ds_add_u64 / ds_min_i64 / ds_max_i64.
//                        A wave tile whose joined rows share one slot goes into the run fold (per
//                        lane u64 sums and i64 min / max, flushed once when the slot changes).
//   k_measures_fold, k_measures_rank, k_measures_dense_write: k_group_fold, k_group_rank and
//                        k_group_dense_write for the wider slot; the rank also adds up the rows.
// sort (everything else): mq_star_positions gives the K joined rows, k_group_star_pack_pos their
//   codes, k_measures_eval_pos one int64 column of K values per measure; mq_index_build sorts the
//   codes, k_group_heads counts the runs; k_measures_seg_write (k_group_seg_write for int64
//   values, one launch a measure) folds the values through the sorted positions.
// The keys of both paths are decoded from the groups' codes by k_group_by_unpack.

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

struct mq_mgroup {
    int path;
    int dev;
    int nkeys, nmeas;
    uint64_t groups;
    hipStream_t stream;  // of the last call that queued work on the buffers below
    // dense: the folded table
    uint32_t range;
    char* tab;
    // sort: the K joined rows' sorted codes, their places among the K, the chunks' head counts, the values [nmeas][K]
    uint64_t k;
    int32_t* sorted;
    unsigned long long* pos;
    uint32_t* ccnt;
    uint32_t blocks;
    uint64_t chunk;
    long long* vals;
    // the tuple behind a code: K_j = klo[j] + (code / kstride[j]) % (krm1[j] + 1)
    int32_t klo[MQ_GROUP_MAX_KEYS];
    uint32_t krm1[MQ_GROUP_MAX_KEYS];
    uint32_t kstride[MQ_GROUP_MAX_KEYS];
};

namespace {

using namespace mqi;
using u64 = unsigned long long;
using i64 = long long;

constexpr int kMaxKeys = MQ_GROUP_MAX_KEYS;
constexpr int kMaxMeas = MQ_GROUP_MAX_MEASURES;
constexpr int kMaxOps = 2 * kMaxMeas;  // distinct operand columns
constexpr uint32_t kNoSlot = ~0u;      // of a row with a component out of bounds: beyond every table
constexpr size_t kDenseLds = 40960;    // what every dense grouping kernel of the library uses: 4 blocks a CU
constexpr int kFoldSlots = 16;
constexpr int kFoldParts = kTPB / kFoldSlots;
constexpr int kSegU = 4;
constexpr int kSegTile = kTPB * kSegU;

constexpr size_t slot_bytes(int nm) { return 4 + 24 * (size_t)nm; }

// The largest power of two of slots whose table fits kDenseLds: 1024, 512, 512, 256.
constexpr uint32_t meas_slots(int nm) {
    uint32_t s = 1;
    while ((size_t)(2 * s) * slot_bytes(nm) <= kDenseLds) s *= 2;
    return s;
}
static_assert(meas_slots(1) == 1024 && meas_slots(2) == 512 && meas_slots(3) == 512 && meas_slots(4) == 256, "dense capacity");

// Tiles in flight per thread. NOT SWEPT: about eight operand loads a lane in flight whatever NM
// (2 * NM columns x tiles), and no more tiles than k_group_star_dense keeps for NT terms; the
// resource report only shows that every instantiation fits 4 waves a SIMD
// without scratch.
constexpr int meas_tiles(int nt, int nm) {
    const int star = nt <= 2 ? 4 : nt == 3 ? 3 : 2;
    const int cap = nm == 1 ? 4 : nm == 2 ? 2 : 1;
    return star < cap ? star : cap;
}

// The measures as kernel arguments: the distinct operand columns and, per measure, which two of
// them it reads (ib == ia for MQ_MEAS_COL) and its op.
struct MeasArgs {
    const int* col[kMaxOps];
    int nd;
    int ia[kMaxMeas], ib[kMaxMeas], op[kMaxMeas];
};

// Exact in int64: |a * b| <= 2^62, |a +- b| < 2^33.
__device__ __forceinline__ i64 meas_eval(int op, int a, int b) {
    return op == MQ_MEAS_COL ? (i64)a : op == MQ_MEAS_ADD ? (i64)a + (i64)b : op == MQ_MEAS_SUB ? (i64)a - (i64)b : (i64)a * (i64)b;
}

__device__ __forceinline__ i64 wave_min_i64(i64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const i64 o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ i64 wave_max_i64(i64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const i64 o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// Column `idx` (grid-uniform) of the ND a lane holds in registers, by and-or under a uniform mask
// (v_and_or_b32): no indexed access, and no select between two loads, which the compiler turns into
// a load through a selected address and with it the whole array into scratch.
template <int ND>
__device__ __forceinline__ int4 pick(const int4 (&c)[ND], int idx) {
    int4 r = make_int4(0, 0, 0, 0);
#pragma unroll
    for (int d = 0; d < ND; d++) {
        const int m = idx == d ? -1 : 0;
        r.x |= c[d].x & m;
        r.y |= c[d].y & m;
        r.z |= c[d].z & m;
        r.w |= c[d].w & m;
    }
    return r;
}

// Operand column `idx` (grid-uniform) of the kernel's arguments, by selects: an indexed read of a
// by-value argument would put the whole struct into scratch.
__device__ __forceinline__ const int* pick_col(const MeasArgs& ma, int idx) {
    const int* r = ma.col[0];
#pragma unroll
    for (int d = 1; d < kMaxOps; d++)
        if (idx == d) r = ma.col[d];
    return r;
}

// The blocks' tables in the scratch: cnt [block][slot]; sum, mn, mx [measure][block][slot]; bad [block][wave].
struct MTabs {
    u64* sum;
    i64* mn;
    i64* mx;
    uint32_t* cnt;
    uint32_t* bad;
};

size_t mtabs_bytes(uint32_t blocks, uint32_t range, int nm) {
    return (size_t)blocks * range * slot_bytes(nm) + (size_t)blocks * kWaves * 4;
}

MTabs mtabs(void* scratch, uint32_t blocks, uint32_t range, int nm) {
    const size_t cells = (size_t)blocks * range;
    MTabs t;
    t.sum = static_cast<u64*>(scratch);
    t.mn = reinterpret_cast<i64*>(t.sum + cells * nm);
    t.mx = t.mn + cells * nm;
    t.cnt = reinterpret_cast<uint32_t*>(t.mx + cells * nm);
    t.bad = t.cnt + cells;
    return t;
}

// The folded table in the handle: [groups][bad][rows][pad] then per slot the count, per measure
// and slot sum, min and max, and per slot the output index.
struct MFinal {
    u64* hdr;
    u64* cnt;
    u64* sum;
    i64* mn;
    i64* mx;
    uint32_t* rank;
};

size_t mfinal_bytes(uint32_t range, int nm) { return 32 + (size_t)range * (12 + 24 * (size_t)nm); }

MFinal mfinal(char* p, uint32_t range, int nm) {
    MFinal f;
    f.hdr = reinterpret_cast<u64*>(p);
    f.cnt = f.hdr + 4;
    f.sum = f.cnt + range;
    f.mn = reinterpret_cast<i64*>(f.sum + (size_t)range * nm);
    f.mx = f.mn + (size_t)range * nm;
    f.rank = reinterpret_cast<uint32_t*>(f.mx + (size_t)range * nm);
    return f;
}

// k_group_star_dense with NM measures in place of the value column. The front half is that
// kernel's, term by term. After the last term the tiles are balloted once more and of each
// distinct operand column only the lines that still hold a joined row are requested, all of the
// iteration's loads before the first use; measure m's value of a row is meas_eval(op, a, b) on
// operands picked from those registers. slot = code, or kNoSlot for a joined row out of bounds,
// which is counted and never used as an address.
template <int NT, int NM, bool VEC>
__global__ __launch_bounds__(kTPB, 4) void k_group_measures_dense(WhereArgs w, StarArgs s, MeasArgs ma, uint64_t n,
                                                                  uint64_t rows_per_block, uint32_t range, MTabs out) {
    constexpr int U = meas_tiles(NT, NM);
    constexpr int ND = 2 * NM;
    constexpr uint32_t kSlots = meas_slots(NM);
    __shared__ uint32_t s_cnt[kSlots];
    __shared__ u64 s_sum[NM][kSlots];
    __shared__ i64 s_mn[NM][kSlots];
    __shared__ i64 s_mx[NM][kSlots];
    const int tid = threadIdx.x, lane = tid & 63;
    for (uint32_t q = tid; q < range; q += kTPB) {  // range <= kSlots: the host checked
        s_cnt[q] = 0u;
#pragma unroll
        for (int m = 0; m < NM; m++) {
            s_sum[m][q] = 0ull;
            s_mn[m][q] = LLONG_MAX;
            s_mx[m][q] = LLONG_MIN;
        }
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
    u64 r_sum[NM];
    i64 r_mn[NM], r_mx[NM];
#pragma unroll
    for (int m = 0; m < NM; m++) {
        r_sum[m] = 0ull;
        r_mn[m] = LLONG_MAX;
        r_mx[m] = LLONG_MIN;
    }

    auto update = [&](uint32_t sl, const i64 (&v)[NM][4], int e) {
        if (sl < range) {  // kNoSlot never is
            atomicAdd(&s_cnt[sl], 1u);
#pragma unroll
            for (int m = 0; m < NM; m++) {
                atomicAdd(&s_sum[m][sl], (u64)v[m][e]);
                atomicMin(&s_mn[m][sl], v[m][e]);
                atomicMax(&s_mx[m][sl], v[m][e]);
            }
        } else {
            nbad++;
        }
    };
    auto flush = [&]() {  // wave-uniform
        const uint32_t c = (uint32_t)wave_sum_u64(r_cnt);  // <= the rows of the block's chunk < 2^31
        u64 sm[NM];
        i64 mn[NM], mx[NM];
#pragma unroll
        for (int m = 0; m < NM; m++) {
            sm[m] = wave_sum_u64(r_sum[m]);
            mn[m] = wave_min_i64(r_mn[m]);
            mx[m] = wave_max_i64(r_mx[m]);
        }
        if (lane == 0) {
            if (run_slot < range) {
                atomicAdd(&s_cnt[run_slot], c);
#pragma unroll
                for (int m = 0; m < NM; m++) {
                    atomicAdd(&s_sum[m][run_slot], sm[m]);
                    atomicMin(&s_mn[m][run_slot], mn[m]);
                    atomicMax(&s_mx[m][run_slot], mx[m]);
                }
            } else {
                nbad += c;
            }
        }
        run_open = false;
        r_cnt = 0;
#pragma unroll
        for (int m = 0; m < NM; m++) {
            r_sum[m] = 0ull;
            r_mn[m] = LLONG_MAX;
            r_mx[m] = LLONG_MIN;
        }
    };
    // k_group_star_dense's consume on the slots of a full tile with a joined row in the wave
    auto consume = [&](uint4 sl, const i64 (&v)[NM][4], uint32_t live, u64 b) {
        const uint32_t sf = live & 1u ? sl.x : live & 2u ? sl.y : live & 4u ? sl.z : sl.w;  // the lane's first joined slot
        const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)sf, __builtin_ctzll(b));
        const bool same = live == 0u || ((!(live & 1u) || sl.x == s0) && (!(live & 2u) || sl.y == s0) &&
                                         (!(live & 4u) || sl.z == s0) && (!(live & 8u) || sl.w == s0));
        if (__all(same)) {  // the joined rows of the wave's 256 share one slot: into the run
            if (run_open && s0 != run_slot) flush();
            run_slot = s0;
            run_open = true;
            r_cnt += (uint32_t)__popc(live);
#pragma unroll
            for (int m = 0; m < NM; m++)
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (live & (1u << e)) {
                        r_sum[m] += (u64)v[m][e];
                        r_mn[m] = v[m][e] < r_mn[m] ? v[m][e] : r_mn[m];
                        r_mx[m] = v[m][e] > r_mx[m] ? v[m][e] : r_mx[m];
                    }
        } else {
            if (live & 1u) update(sl.x, v, 0);
            if (live & 2u) update(sl.y, v, 1);
            if (live & 4u) update(sl.z, v, 2);
            if (live & 8u) update(sl.w, v, 3);
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
        int4 c[T][ND];
#pragma unroll
        for (int u = 0; u < T; u++) {
            b[u] = __ballot(live[u] != 0u);
#pragma unroll
            for (int d = 0; d < ND; d++) {
                c[u][d] = make_int4(0, 0, 0, 0);
                if (d < ma.nd && b[u] != 0 && line_live(b[u], lane)) c[u][d] = load4_nt<VEC>(ma.col[d] + row + (uint64_t)u * kTileRows);
            }
        }
#pragma unroll
        for (int u = 0; u < T; u++) {
            if (b[u] == 0) continue;  // wave-uniform
            i64 v[NM][4];
#pragma unroll
            for (int m = 0; m < NM; m++) {
                const int4 x = pick<ND>(c[u], ma.ia[m]), y = pick<ND>(c[u], ma.ib[m]);
                v[m][0] = meas_eval(ma.op[m], x.x, y.x);
                v[m][1] = meas_eval(ma.op[m], x.y, y.y);
                v[m][2] = meas_eval(ma.op[m], x.z, y.z);
                v[m][3] = meas_eval(ma.op[m], x.w, y.w);
            }
            consume(make_uint4(in[u] & 1u ? code[u].x : kNoSlot, in[u] & 2u ? code[u].y : kNoSlot, in[u] & 4u ? code[u].z : kNoSlot,
                               in[u] & 8u ? code[u].w : kNoSlot),
                    v, live[u], b[u]);
        }
    };

    uint64_t t = start;
    for (; t + (uint64_t)U * kTileRows <= end; t += (uint64_t)U * kTileRows) tiles(std::integral_constant<int, U>{}, t);
    for (; t + kTileRows <= end; t += kTileRows) tiles(std::integral_constant<int, 1>{}, t);
    if (t < end) {  // the column's ragged tile: row by row, none past the end
        const uint64_t row = t + (uint64_t)tid * 4;
        const uint32_t live = live_ragged(w, row, end);
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
            if (!joined) continue;
            i64 v[NM][4];
#pragma unroll
            for (int m = 0; m < NM; m++) {
                v[m][0] = meas_eval(ma.op[m], pick_col(ma, ma.ia[m])[row + i], pick_col(ma, ma.ib[m])[row + i]);
                v[m][1] = v[m][2] = v[m][3] = 0;
            }
            update(ok ? code : kNoSlot, v, 0);
        }
    }
    if (run_open) flush();
    nbad = (uint32_t)wave_sum_u64(nbad);
    if (lane == 0) out.bad[(size_t)blockIdx.x * kWaves + (tid >> 6)] = nbad;
    __syncthreads();
    const size_t cells = (size_t)gridDim.x * range;
    const size_t base = (size_t)blockIdx.x * range;
    for (uint32_t q = tid; q < range; q += kTPB) {
        out.cnt[base + q] = s_cnt[q];
#pragma unroll
        for (int m = 0; m < NM; m++) {
            out.sum[m * cells + base + q] = s_sum[m][q];
            out.mn[m * cells + base + q] = s_mn[m][q];
            out.mx[m * cells + base + q] = s_mx[m][q];
        }
    }
}

// Per slot, the blocks' tables combined (k_group_fold's shape: 16 slots x 16 block strides a
// workgroup, the strides combined through LDS), measure by measure.
__global__ __launch_bounds__(kTPB) void k_measures_fold(MTabs in, uint32_t blocks, uint32_t range, int nm, MFinal f) {
    __shared__ u64 p_a[kFoldParts][kFoldSlots];
    __shared__ i64 p_mn[kFoldParts][kFoldSlots];
    __shared__ i64 p_mx[kFoldParts][kFoldSlots];
    const uint32_t sl = threadIdx.x % kFoldSlots, part = threadIdx.x / kFoldSlots;
    const uint32_t s = blockIdx.x * kFoldSlots + sl;
    const size_t cells = (size_t)blocks * range;
    u64 c = 0;
    if (s < range)
        for (uint32_t b = part; b < blocks; b += kFoldParts) c += in.cnt[(size_t)b * range + s];
    p_a[part][sl] = c;
    __syncthreads();
    if (part == 0 && s < range) {
        for (int p = 1; p < kFoldParts; p++) c += p_a[p][sl];
        f.cnt[s] = c;
    }
    for (int m = 0; m < nm; m++) {  // block-uniform trip count
        u64 sm = 0;
        i64 mn = LLONG_MAX, mx = LLONG_MIN;
        if (s < range)
            for (uint32_t b = part; b < blocks; b += kFoldParts) {
                const size_t i = m * cells + (size_t)b * range + s;
                sm += in.sum[i];
                mn = in.mn[i] < mn ? in.mn[i] : mn;
                mx = in.mx[i] > mx ? in.mx[i] : mx;
            }
        __syncthreads();  // the previous round's reads are done
        p_a[part][sl] = sm;
        p_mn[part][sl] = mn;
        p_mx[part][sl] = mx;
        __syncthreads();
        if (part == 0 && s < range) {
            for (int p = 1; p < kFoldParts; p++) {
                sm += p_a[p][sl];
                mn = p_mn[p][sl] < mn ? p_mn[p][sl] : mn;
                mx = p_mx[p][sl] > mx ? p_mx[p][sl] : mx;
            }
            f.sum[(size_t)m * range + s] = sm;
            f.mn[(size_t)m * range + s] = mn;
            f.mx[(size_t)m * range + s] = mx;
        }
    }
}

// One block: rank[s] = non-empty slots below s, hdr[0] = their number, hdr[1] = the joined rows
// the blocks found outside the bounds, hdr[2] = the sum of the slots' counts.
__global__ __launch_bounds__(kTPB) void k_measures_rank(MFinal f, uint32_t range, const uint32_t* __restrict__ bad, uint32_t nbad) {
    __shared__ uint32_t s_w[kWaves];
    __shared__ u64 s_b[kWaves], s_r[kWaves];
    constexpr uint32_t kPer = meas_slots(1) / kTPB;
    const uint32_t s0 = threadIdx.x * kPer;
    uint32_t c = 0;
    u64 rows = 0;
#pragma unroll
    for (uint32_t e = 0; e < kPer; e++)
        if (s0 + e < range) {
            c += f.cnt[s0 + e] != 0;
            rows += f.cnt[s0 + e];
        }
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
    rows = wave_sum_u64(rows);
    if ((threadIdx.x & 63) == 0) {
        s_b[threadIdx.x >> 6] = b;
        s_r[threadIdx.x >> 6] = rows;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        f.hdr[0] = total;
        f.hdr[1] = s_b[0] + s_b[1] + s_b[2] + s_b[3];
        f.hdr[2] = s_r[0] + s_r[1] + s_r[2] + s_r[3];
    }
}

// Where a write puts the measures' aggregates: NULL entries are skipped.
struct MOuts {
    u64* sum[kMaxMeas];
    i64* mn[kMaxMeas];
    i64* mx[kMaxMeas];
};

__global__ __launch_bounds__(kTPB) void k_measures_dense_write(MFinal f, uint32_t range, int nm, int32_t* __restrict__ codes_out,
                                                               u64* __restrict__ count_out, MOuts o) {
    const uint32_t s = blockIdx.x * kTPB + threadIdx.x;
    if (s >= range) return;
    const u64 c = f.cnt[s];
    if (c == 0) return;
    const uint32_t g = f.rank[s];  // < the group count the plan returned
    if (codes_out) codes_out[g] = (int32_t)s;
    if (count_out) count_out[g] = c;
#pragma unroll
    for (int m = 0; m < kMaxMeas; m++) {
        if (m >= nm) continue;
        if (o.sum[m]) o.sum[m][g] = f.sum[(size_t)m * range + s];
        if (o.mn[m]) o.mn[m][g] = f.mn[(size_t)m * range + s];
        if (o.mx[m]) o.mx[m][g] = f.mx[(size_t)m * range + s];
    }
}

// ---- the sort path ----

// out[m][i] = measure m of row pos[i] for the k joined rows of mq_star_positions (grid-stride); a
// position outside [0, n), which mq_star_positions never writes, reads nothing and leaves 0.
__global__ __launch_bounds__(kTPB) void k_measures_eval_pos(MeasArgs ma, int nm, const int32_t* __restrict__ pos, uint32_t k,
                                                            uint32_t n, i64* __restrict__ out) {
    for (u64 i = (u64)blockIdx.x * kTPB + threadIdx.x; i < k; i += (u64)gridDim.x * kTPB) {
        const uint32_t p = (uint32_t)pos[i];
        int v[kMaxOps];
#pragma unroll
        for (int d = 0; d < kMaxOps; d++) v[d] = d < ma.nd && p < n ? ma.col[d][p] : 0;
#pragma unroll
        for (int m = 0; m < kMaxMeas; m++) {
            if (m >= nm) continue;
            int a = v[0], b = v[0];
#pragma unroll
            for (int d = 1; d < kMaxOps; d++) {
                if (ma.ia[m] == d) a = v[d];
                if (ma.ib[m] == d) b = v[d];
            }
            out[(size_t)m * k + i] = meas_eval(ma.op[m], a, b);
        }
    }
}

// One launch of k_measures_seg_write: the codes and counts (either may be NULL) and one measure.
struct MSegOut {
    int32_t* codes;
    u64* count;
    u64* sum;
    i64* mn;
    i64* mx;
    u64 groups;
};

// One block (k_group_seg_init): the group open at the end of a chunk is the only one that rows of
// several chunks can belong to: it receives the identity in every output that is wanted.
__global__ __launch_bounds__(kTPB) void k_measures_seg_init(const uint32_t* __restrict__ ccnt, uint32_t blocks, u64 groups,
                                                            u64* __restrict__ count, int nm, MOuts o) {
    __shared__ uint32_t s_w[kWaves];
    u64 run = 0;
    for (uint32_t b0 = 0; b0 < blocks; b0 += kTPB) {  // block-uniform trip count
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t v = b < blocks ? ccnt[b] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_scan(v, s_w, &total);
        const u64 incl = run + ex + v;
        if (b < blocks && incl > 0 && incl <= groups) {
            const u64 g = incl - 1;
            if (count) count[g] = 0ull;
#pragma unroll
            for (int m = 0; m < kMaxMeas; m++) {
                if (m >= nm) continue;
                if (o.sum[m]) o.sum[m][g] = 0ull;
                if (o.mn[m]) o.mn[m][g] = LLONG_MAX;
                if (o.mx[m]) o.mx[m][g] = LLONG_MIN;
            }
        }
        run += total;
    }
}

struct MRun {  // one run's aggregate while it is open
    u64 cnt;
    u64 sum;
    i64 mn, mx;
};

__device__ __forceinline__ void emit_run(const MSegOut& o, u64 g, const MRun& r, bool atomic) {
    if (g >= o.groups) return;  // never: g counts heads, the plan counted the same heads
    if (atomic) {
        if (o.count) atomicAdd(o.count + g, r.cnt);
        if (o.sum) atomicAdd(o.sum + g, r.sum);
        if (o.mn) atomicMin(o.mn + g, r.mn);
        if (o.mx) atomicMax(o.mx + g, r.mx);
    } else {
        if (o.count) o.count[g] = r.cnt;
        if (o.sum) o.sum[g] = r.sum;
        if (o.mn) o.mn[g] = r.mn;
        if (o.mx) o.mx[g] = r.mx;
    }
}

// k_group_seg_write over one int64 value column: row i of the sorted codes belongs to group
// (heads in [0, i]) - 1; within a tile, local slot l = heads in the tile up to and including the
// row: slot 0 continues the run open before the tile, slot nh is open at its end.
__global__ __launch_bounds__(kTPB) void k_measures_seg_write(const int32_t* __restrict__ sorted, const u64* __restrict__ pos,
                                                             const i64* __restrict__ vals, uint32_t n, uint64_t chunk,
                                                             const uint32_t* __restrict__ ccnt, int need_vals, MSegOut o) {
    __shared__ uint32_t s_c[kSegTile + 1];
    __shared__ u64 s_s[kSegTile + 1];
    __shared__ i64 s_mn[kSegTile + 1];
    __shared__ i64 s_mx[kSegTile + 1];
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint32_t s_hc[kSegU][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t below = 0;
    for (uint32_t i = tid; i < blockIdx.x; i += kTPB) below += ccnt[i];
    u64 base = block_sum(below, s_w);  // heads before the tile (< 2^31)
    const uint64_t i0 = (uint64_t)blockIdx.x * chunk;
    const uint64_t i1 = i0 + chunk < n ? i0 + chunk : n;
    // thread 0 keeps the open run: its group, and whether it began before this chunk
    MRun car = {0ull, 0ull, LLONG_MAX, LLONG_MIN};
    u64 car_g = 0;
    bool car_valid = false, car_left = false;
    for (uint64_t s = i0; s < i1; s += kSegTile) {  // block-uniform trip count
        for (uint32_t q = tid; q <= (uint32_t)kSegTile; q += kTPB) {
            s_c[q] = 0u;
            s_s[q] = 0ull;
            s_mn[q] = LLONG_MAX;
            s_mx[q] = LLONG_MIN;
        }
        int32_t k[kSegU];
        i64 v[kSegU];
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
                atomicAdd(&s_s[l], (u64)v[u]);
                atomicMin(&s_mn[l], v[u]);
                atomicMax(&s_mx[l], v[u]);
            }
            if (h[u] && o.codes && base + l - 1 < o.groups) o.codes[base + l - 1] = k[u];
        }
        __syncthreads();
        for (uint32_t q = 1 + tid; q < nh; q += kTPB)  // runs that begin and end in this tile
            emit_run(o, base + q - 1, MRun{s_c[q], s_s[q], s_mn[q], s_mx[q]}, false);
        if (tid == 0) {
            if (s_c[0]) {  // rows of the run open before the tile
                if (!car_valid) {  // the chunk's first tile, whose first row is no head
                    car_valid = car_left = true;
                    car_g = base - 1;
                }
                car.cnt += s_c[0];
                car.sum += s_s[0];
                car.mn = s_mn[0] < car.mn ? s_mn[0] : car.mn;
                car.mx = s_mx[0] > car.mx ? s_mx[0] : car.mx;
            }
            if (nh) {  // a head closed it; the tile's last run is open now
                if (car_valid) emit_run(o, car_g, car, car_left);
                car = MRun{s_c[nh], s_s[nh], s_mn[nh], s_mx[nh]};
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

template <int NT, int NM, bool VEC>
int launch_measures_dense(const DevState* s, const WhereArgs& w, const StarArgs& a, const MeasArgs& ma, uint64_t n, uint32_t range,
                          void** scratch_out, MTabs* tabs, uint32_t* blocks_out, hipStream_t st) {
    uint32_t g;
    uint64_t rpb;
    geometry(s, n, reinterpret_cast<const void*>(&k_group_measures_dense<NT, NM, VEC>), &g, &rpb,
             (uint64_t)meas_tiles(NT, NM) * kTileRows);
    void* scratch = pool_alloc(mtabs_bytes(g, range, NM));
    if (!scratch) return set_err(MQ_ENOMEM, "mq_group_measures_plan: scratch allocation failed");
    *tabs = mtabs(scratch, g, range, NM);
    *scratch_out = scratch;
    *blocks_out = g;
    hipLaunchKernelGGL((k_group_measures_dense<NT, NM, VEC>), dim3(g), dim3(kTPB), 0, st, w, a, ma, n, rpb, range, *tabs);
    LAUNCHCHK("k_group_measures_dense");
    return MQ_OK;
}

// The dense path: the stream, the fold, the rank; *rows = the joined rows.
int plan_dense(const DevState* s, mq_mgroup* g, const WhereArgs& w, const StarArgs& a, const MeasArgs& ma, bool vec, uint64_t n,
               uint64_t* rows, hipStream_t st) {
    const char* who = "mq_group_measures_plan";
    const int nm = g->nmeas;
    g->tab = static_cast<char*>(pool_alloc(mfinal_bytes(g->range, nm)));
    if (!g->tab) return set_err(MQ_ENOMEM, "%s: table allocation failed", who);
    const MFinal f = mfinal(g->tab, g->range, nm);
    void* scratch = nullptr;
    MTabs tabs;
    uint32_t blocks = 0;
    auto with_nm = [&](auto nt, auto nmc) {
        constexpr int NT = decltype(nt)::value, NM = decltype(nmc)::value;
        return vec ? launch_measures_dense<NT, NM, true>(s, w, a, ma, n, g->range, &scratch, &tabs, &blocks, st)
                   : launch_measures_dense<NT, NM, false>(s, w, a, ma, n, g->range, &scratch, &tabs, &blocks, st);
    };
    auto with_nt = [&](auto nt) {
        return nm == 1   ? with_nm(nt, std::integral_constant<int, 1>{})
               : nm == 2 ? with_nm(nt, std::integral_constant<int, 2>{})
               : nm == 3 ? with_nm(nt, std::integral_constant<int, 3>{})
                         : with_nm(nt, std::integral_constant<int, 4>{});
    };
    int rc = a.nterms == 1   ? with_nt(std::integral_constant<int, 1>{})
             : a.nterms == 2 ? with_nt(std::integral_constant<int, 2>{})
             : a.nterms == 3 ? with_nt(std::integral_constant<int, 3>{})
                             : with_nt(std::integral_constant<int, 4>{});
    if (rc) {
        pool_free_on(scratch, st);
        return rc;
    }
    hipLaunchKernelGGL(k_measures_fold, dim3((g->range + kFoldSlots - 1) / kFoldSlots), dim3(kTPB), 0, st, tabs, blocks, g->range, nm, f);
    hipLaunchKernelGGL(k_measures_rank, dim3(1), dim3(kTPB), 0, st, f, g->range, tabs.bad, blocks * kWaves);
    const hipError_t e = hipGetLastError();
    pool_free_on(scratch, st);  // the two kernels queued above are its last readers
    u64 h[3] = {0, 0, 0};
    rc = e == hipSuccess ? MQ_OK : set_err(MQ_EHIP, "launch of k_measures_fold / k_measures_rank failed: %s", hipGetErrorString(e));
    if (!rc && hipMemcpyAsync(h, f.hdr, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess)
        rc = set_err(MQ_EHIP, "%s: header download failed", who);
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = set_err(MQ_EHIP, "%s: stream failed", who);
    if (rc) return rc;
    if (h[1]) return set_err(MQ_EINVAL, "%s: %llu joined rows with a component outside its bounds", who, h[1]);
    g->groups = h[0];
    *rows = h[2];
    return MQ_OK;
}

void release(mq_mgroup* g, hipStream_t st) {
    pool_free_on(g->tab, st);
    pool_free_on(g->sorted, st);
    pool_free_on(g->pos, st);
    pool_free_on(g->ccnt, st);
    pool_free_on(g->vals, st);
    delete g;
}

}  // namespace

extern "C" {

uint32_t mq_group_measures_dense_slots(int nmeas) { return nmeas < 1 || nmeas > kMaxMeas ? 0u : meas_slots(nmeas); }

int mq_group_measures_auto_path(const int32_t* h_key_bounds, int nkeys, int nmeas, uint64_t* h_space) {
    const char* who = "mq_group_measures_auto_path";
    if (h_space) *h_space = 0;
    if (nkeys < 1 || nkeys > kMaxKeys) return set_err(MQ_EINVAL, "%s: nkeys %d outside 1..%d", who, nkeys, kMaxKeys);
    if (nmeas < 1 || nmeas > kMaxMeas) return set_err(MQ_EINVAL, "%s: nmeas %d outside 1..%d", who, nmeas, kMaxMeas);
    if (!h_key_bounds) return set_err(MQ_EINVAL, "%s: NULL pointer", who);
    uint64_t space;
    if (!group_key_space(h_key_bounds, nkeys, &space)) return set_err(MQ_EINVAL, "%s: a component's bounds are empty", who);
    if (h_space) *h_space = space;
    if (space > (1ull << 32)) return set_err(MQ_EINVAL, "%s: the key space %llu is wider than 2^32", who, (u64)space);
    return space <= meas_slots(nmeas) ? MQ_GROUP_DENSE : MQ_GROUP_SORT;
}

int mq_group_measures_plan(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols, const mq_star_term* h_terms, int nterms,
                           const mq_measure* h_meas, int nmeas, uint64_t n, const int32_t* h_key_bounds, int path, mq_mgroup** out,
                           uint64_t* h_groups, int* h_path, uint64_t* h_rows, void* stream) {
    const char* who = "mq_group_measures_plan";
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (out) *out = nullptr;
    if (h_groups) *h_groups = 0;
    if (h_rows) *h_rows = 0;
    if (nterms < 1 || nterms > MQ_STAR_MAX_TERMS) return set_err(MQ_EINVAL, "%s: nterms %d outside 1..%d", who, nterms, (int)MQ_STAR_MAX_TERMS);
    if (nmeas < 1 || nmeas > kMaxMeas) return set_err(MQ_EINVAL, "%s: nmeas %d outside 1..%d", who, nmeas, kMaxMeas);
    if (!out || !h_groups || !h_terms || !h_meas || (ncols > 0 && (!d_cols || !h_ranges))) return set_err(MQ_EINVAL, "%s: NULL pointer", who);
    int nkeys = 0;
    for (int j = 0; j < nterms; j++) {
        if (h_terms[j].km && h_terms[j].ks) return set_err(MQ_EINVAL, "%s: term %d has both a key map and a key set", who, j);
        nkeys += h_terms[j].ks ? 0 : 1;
    }
    if (nkeys < 1 || nkeys > kMaxKeys) return set_err(MQ_EINVAL, "%s: %d components outside 1..%d", who, nkeys, kMaxKeys);
    if (ncols < 0 || ncols > MQ_WHERE_MAX_COLS) return set_err(MQ_EINVAL, "%s: ncols %d outside 0..%d", who, ncols, (int)MQ_WHERE_MAX_COLS);
    if (path != MQ_GROUP_AUTO && path != MQ_GROUP_DENSE && path != MQ_GROUP_SORT) return set_err(MQ_EINVAL, "%s: path %d", who, path);
    if (n >= (1ull << 31)) return set_err(MQ_EINVAL, "%s: n >= 2^31", who);
    for (int m = 0; m < nmeas; m++) {
        const mq_measure& q = h_meas[m];
        if (q.op != MQ_MEAS_COL && q.op != MQ_MEAS_ADD && q.op != MQ_MEAS_SUB && q.op != MQ_MEAS_MUL)
            return set_err(MQ_EINVAL, "%s: measure %d: op %d", who, m, q.op);
        if (q.reserved != 0) return set_err(MQ_EINVAL, "%s: measure %d: reserved must be 0", who, m);
        if (q.op == MQ_MEAS_COL && q.d_b) return set_err(MQ_EINVAL, "%s: measure %d: d_b must be NULL for MQ_MEAS_COL", who, m);
        if (q.op != MQ_MEAS_COL && !q.d_b) return set_err(MQ_EINVAL, "%s: measure %d: a binary op needs d_b", who, m);
    }
    const uint32_t slots = meas_slots(nmeas);
    int32_t b[2 * kMaxKeys];
    uint64_t space = 0;
    // the bounds given, checked before anything is allocated; bounds the plan finds, after it found them
    auto check_space = [&]() {
        if (!group_key_space(b, nkeys, &space)) return set_err(MQ_EINVAL, "%s: a component's bounds are empty", who);
        if (space > (1ull << 32))
            return set_err(MQ_EINVAL, "%s: the key space %llu (saturated at 2^63) is wider than 2^32", who, (u64)space);
        if (path == MQ_GROUP_DENSE && space > slots)
            return set_err(MQ_EINVAL, "%s: the key space %llu exceeds the dense path's %u slots with %d measures", who, (u64)space, slots, nmeas);
        return (int)MQ_OK;
    };
    if (n) {
        for (int c = 0; c < ncols; c++)
            if (!d_cols[c] || (reinterpret_cast<uintptr_t>(d_cols[c]) & 3u))
                return set_err(MQ_EINVAL, "%s: column %d NULL or not 4-byte aligned", who, c);
        for (int j = 0; j < nterms; j++)
            if (!h_terms[j].d_col || (reinterpret_cast<uintptr_t>(h_terms[j].d_col) & 3u))
                return set_err(MQ_EINVAL, "%s: term %d: column NULL or not 4-byte aligned", who, j);
        for (int m = 0; m < nmeas; m++)
            if (!h_meas[m].d_a || (reinterpret_cast<uintptr_t>(h_meas[m].d_a) & 3u) || (reinterpret_cast<uintptr_t>(h_meas[m].d_b) & 3u))
                return set_err(MQ_EINVAL, "%s: measure %d: column NULL or not 4-byte aligned", who, m);
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
    mq_mgroup* g = new (std::nothrow) mq_mgroup();
    if (!g) return set_err(MQ_ENOMEM, "%s: out of host memory", who);
    g->dev = dev;
    g->stream = st;
    g->nkeys = nkeys;
    g->nmeas = nmeas;
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
    g->path = path != MQ_GROUP_AUTO ? path : space <= slots ? MQ_GROUP_DENSE : MQ_GROUP_SORT;
    // the terms as the kernels take them; the tuple's code as mq_group_star_plan lays it out, kept for the write
    StarArgs a = {};
    a.nterms = nterms;
    bool vec = wvec;
    {
        uint64_t stride = 1;  // up to the key space
        for (int j = nterms - 1, c = nkeys - 1; j >= 0; j--) {
            StarTerm& t = a.t[j];
            const mq_keyset* ks = h_terms[j].km ? h_terms[j].km->ks : h_terms[j].ks;
            t.col = h_terms[j].d_col;
            vec = vec && aligned16(t.col);
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
            g->klo[c] = b[2 * c];
            g->krm1[c] = t.rm1;
            g->kstride[c] = t.stride;
            stride *= (uint64_t)t.rm1 + 1;
            c--;
        }
    }
    // the distinct operand columns, each loaded once; the measures index into the list
    MeasArgs ma = {};
    auto operand = [&](const int32_t* p) {
        for (int d = 0; d < ma.nd; d++)
            if (ma.col[d] == p) return d;
        ma.col[ma.nd] = p;
        vec = vec && aligned16(p);
        return ma.nd++;
    };
    for (int m = 0; m < nmeas; m++) {
        ma.op[m] = h_meas[m].op;
        ma.ia[m] = operand(h_meas[m].d_a);
        ma.ib[m] = h_meas[m].op == MQ_MEAS_COL ? ma.ia[m] : operand(h_meas[m].d_b);
    }
    uint64_t rows = 0;
    if (g->path == MQ_GROUP_DENSE) {
        g->range = (uint32_t)space;
        rc = plan_dense(s, g, w, a, ma, vec, n, &rows, st);
        if (rc) return fail(rc);
    } else {
        // the K joined rows' positions, their codes packed and their measures evaluated through them, then the sort
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
            g->vals = static_cast<i64*>(pool_alloc(k * 8 * (size_t)nmeas));
            d_total = static_cast<u64*>(pool_alloc(sizeof(u64)));
            const uint32_t grid = stream_grid(s, (k + 3) / 4);  // four rows a lane in flight
            bad = static_cast<uint32_t*>(pool_alloc((size_t)grid * kWaves * 4));
            if (!packed || !g->vals || !d_total || !bad) rc = set_err(MQ_ENOMEM, "%s: allocation failed", who);
            if (!rc) {
                group_launch_star_pack_pos(a, grid, pos, (uint32_t)k, (uint32_t)n, 0x80000000u, packed, bad, st);
                group_launch_bad_total(bad, grid * kWaves, d_total, st);
                hipLaunchKernelGGL(k_measures_eval_pos, dim3(stream_grid(s, k)), dim3(kTPB), 0, st, ma, nmeas, pos, (uint32_t)k,
                                   (uint32_t)n, g->vals);
                if (hipGetLastError() != hipSuccess)
                    rc = set_err(MQ_EHIP, "launch of k_group_star_pack_pos / k_group_by_bad / k_measures_eval_pos failed");
            }
            u64 total = 0;
            if (!rc && hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, st) != hipSuccess)
                rc = set_err(MQ_EHIP, "%s: count download failed", who);
            if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = set_err(MQ_EHIP, "%s: stream failed", who);
            if (!rc && total) rc = set_err(MQ_EINVAL, "%s: %llu joined rows with a component outside its bounds", who, total);
        }
        pool_free(bad);
        pool_free(d_total);
        pool_free_on(pos, st);  // the pack and the evaluation queued above are its last readers
        if (!rc && k) {
            g->k = k;
            g->sorted = static_cast<int32_t*>(pool_alloc(k * 4));
            g->pos = static_cast<u64*>(pool_alloc(k * 8));
            g->ccnt = static_cast<uint32_t*>(pool_alloc(16 + (size_t)kMaxBlocks * 4));  // [groups u64][pad] then the counts
            if (!g->sorted || !g->pos || !g->ccnt) rc = set_err(MQ_ENOMEM, "%s: allocation failed", who);
            if (!rc) rc = mq_index_build(packed, k, g->sorted, reinterpret_cast<uint64_t*>(g->pos), stream);  // synchronises
            if (!rc) {
                mq_group_sort_geometry(k, &g->blocks, &g->chunk);
                if (g->blocks > (uint32_t)kMaxBlocks) rc = set_err(MQ_EHIP, "%s: the sort path's grid of %u chunks", who, g->blocks);
            }
            u64* hdr = reinterpret_cast<u64*>(g->ccnt);
            u64 groups = 0;
            if (!rc && hipMemsetAsync(hdr, 0, 16, st) != hipSuccess) rc = set_err(MQ_EHIP, "%s: memset failed", who);
            if (!rc) {
                group_launch_heads(g->sorted, (uint32_t)k, g->chunk, g->blocks, g->ccnt + 4, hdr, st);
                if (hipGetLastError() != hipSuccess) rc = set_err(MQ_EHIP, "launch of k_group_heads failed");
            }
            if (!rc && hipMemcpyAsync(&groups, hdr, 8, hipMemcpyDeviceToHost, st) != hipSuccess)
                rc = set_err(MQ_EHIP, "%s: count download failed", who);
            if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = set_err(MQ_EHIP, "%s: stream failed", who);
            g->groups = groups;
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

int mq_group_measures_write(mq_mgroup* g, int32_t* const* d_keys_out, uint64_t* d_count_out, int64_t* const* d_sum_out,
                            int64_t* const* d_min_out, int64_t* const* d_max_out, void* stream) {
    const char* who = "mq_group_measures_write";
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!g) return set_err(MQ_EINVAL, "%s: NULL handle", who);
    int dev = -1;
    if ((rc = current_device(&dev))) return rc;
    if (dev != g->dev) return set_err(MQ_EINVAL, "%s: the plan was made on device %d", who, g->dev);
    if (g->groups == 0) return MQ_OK;
    hipStream_t st = (hipStream_t)stream;
    g->stream = st;
    int32_t* keys[kMaxKeys] = {};
    bool want_keys = false;
    for (int j = 0; j < g->nkeys; j++) {
        keys[j] = d_keys_out ? d_keys_out[j] : nullptr;
        want_keys = want_keys || keys[j];
    }
    MOuts o = {};
    for (int m = 0; m < g->nmeas; m++) {
        o.sum[m] = d_sum_out ? reinterpret_cast<u64*>(d_sum_out[m]) : nullptr;
        o.mn[m] = d_min_out ? reinterpret_cast<i64*>(d_min_out[m]) : nullptr;
        o.mx[m] = d_max_out ? reinterpret_cast<i64*>(d_max_out[m]) : nullptr;
    }
    u64* cnt = reinterpret_cast<u64*>(d_count_out);
    int32_t* codes = nullptr;  // the groups' slots or sorted codes
    if (want_keys && !(codes = static_cast<int32_t*>(pool_alloc(g->groups * 4)))) return set_err(MQ_ENOMEM, "%s: allocation failed", who);
    if (g->path == MQ_GROUP_DENSE) {
        hipLaunchKernelGGL(k_measures_dense_write, dim3((g->range + kTPB - 1) / kTPB), dim3(kTPB), 0, st,
                           mfinal(g->tab, g->range, g->nmeas), g->range, g->nmeas, codes, cnt, o);
    } else {
        hipLaunchKernelGGL(k_measures_seg_init, dim3(1), dim3(kTPB), 0, st, g->ccnt + 4, g->blocks, (u64)g->groups, cnt, g->nmeas, o);
        bool first = true;  // the first launch also writes the codes and the counts
        for (int m = 0; m < g->nmeas; m++) {
            if (!o.sum[m] && !o.mn[m] && !o.mx[m]) continue;
            const MSegOut so = {first ? codes : nullptr, first ? cnt : nullptr, o.sum[m], o.mn[m], o.mx[m], (u64)g->groups};
            hipLaunchKernelGGL(k_measures_seg_write, dim3(g->blocks), dim3(kTPB), 0, st, g->sorted, g->pos, g->vals + (size_t)m * g->k,
                               (uint32_t)g->k, g->chunk, g->ccnt + 4, 1, so);
            first = false;
        }
        if (first && (codes || cnt)) {
            const MSegOut so = {codes, cnt, nullptr, nullptr, nullptr, (u64)g->groups};
            hipLaunchKernelGGL(k_measures_seg_write, dim3(g->blocks), dim3(kTPB), 0, st, g->sorted, g->pos, g->vals, (uint32_t)g->k,
                               g->chunk, g->ccnt + 4, 0, so);
        }
    }
    if (codes)
        group_launch_unpack(codes, g->groups, g->klo, g->krm1, g->kstride, g->nkeys, g->path == MQ_GROUP_DENSE ? 0u : 0x80000000u, keys,
                            stream_grid(s, g->groups), st);
    if (hipGetLastError() != hipSuccess) rc = set_err(MQ_EHIP, "%s: a launch failed", who);
    pool_free_on(codes, st);  // k_group_by_unpack is its last reader
    return rc;
}

int mq_group_measures_free(mq_mgroup* g) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!g) return MQ_OK;
    release(g, g->stream);  // a queued write may still read the buffers: freed in its stream's order
    return MQ_OK;
}

}  // extern "C"
