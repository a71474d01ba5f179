// mq_dml.hip — row deletes, updates and inserts on resident tables.
//
// The reference's workload generator has a fifth milestone (tests 38-43) whose DSL
// deletes and updates rows by a position list: relational_delete(db1.tbl5,d1) and
// relational_update(db1.tbl5.col1,u1,-10). The reference server has no branch for them
// (parse.c:876-960), so the semantics are the generator's own pandas statements
// (milestone5.py:127-142, 186-202): an update assigns one value to the listed rows of
// one column; a delete drops the listed rows from every column and the survivors keep
// their order.
//
// A delete is a plan and two apply steps on one workspace:
//   k_dml_mark        : one bit per row, set with a vector atomic OR for every listed id
//                       (any order, repeats allowed); ids outside [0, n) are counted.
//   k_dml_word_sums,
//   k_dml_word_prefix : the exclusive count of deleted rows before each 64-bit bitmap
//                       word (u32, n < 2^31), by a fixed grid of contiguous chunks:
//                       chunk sums first, then every block adds the sums of the chunks
//                       below it and scans its own words. No block waits for another.
//   k_dml_compact     : one block per (4096-row tile, column). A row r that survives
//                       goes to r - (prefix[r / 64] + popcount(word & bits below r)):
//                       every offset follows from the bitmap alone. The tile's survivors
//                       are gathered in LDS, placed so that LDS index and output address
//                       agree modulo 16 bytes, and leave as dwordx4 stores.
//   k_dml_index_count,
//   k_dml_index_write : a sorted index's entries whose row survives, in their order, the
//                       positions renumbered by the same rank. The predicate is a gather
//                       into the bitmap, so this is count -> prefix -> write, again over
//                       contiguous chunks of a fixed grid.
// An update is one scatter (k_dml_update).
//
// An insert is the inverse: the bitmap lies over the n + k OUTPUT slots,
// a set bit marks a slot that a new row takes, and the same word prefix gives rank1(s),
// the new rows before slot s. Output slot s then holds new[rank1(s)] or old[s - rank1(s)]:
//   k_ins_points      : the insertion point of every (sorted) new value, an upper bound
//                       by binary search;
//   k_ins_mark        : the j-th new row takes slot ins[j] + j; points that descend or
//                       exceed n are counted;
//   k_dml_expand      : one block per (4096-slot tile, column). The tile's old rows and
//                       its new rows are each one contiguous source range; both are staged
//                       in LDS by dwordx4 loads of whole 16-byte lines and leave
//                       interleaved as dwordx4 stores;
//   k_ins_index       : the same expansion over a sorted index's values and positions,
//                       old positions renumbered by a search in the table's points.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mq_common.h"
#include "mq_device.h"
#include "mq_scan_common.h"

namespace {

using namespace mqi;
using u64 = unsigned long long;

constexpr int kDelTile = 4096;              // rows per compaction block: 4 dwordx4 per lane
constexpr int kDelWords = kDelTile / 64;    // bitmap words per tile
constexpr int kRankBlocks = 1024;           // chunks of the word-prefix pass
constexpr int kIdxBlocks = 2048;            // chunks of the index pass (one resident round)
constexpr int kIdxU = 4;                    // index entries per lane per step
constexpr int kIdxStep = kTPB * kIdxU;
constexpr int kColsPerLaunch = 64;          // column pointers carried as kernel arguments
constexpr size_t kHdrBytes = 64;            // [bad u64][deleted u64]

struct ColPtrs {
    const int32_t* in[kColsPerLaunch];
    int32_t* out[kColsPerLaunch];
};

struct InsPtrs {
    const int32_t* old_rows[kColsPerLaunch];
    const int32_t* new_rows[kColsPerLaunch];
    int32_t* out[kColsPerLaunch];
};

// Where the plan's pieces lie in the workspace, from n alone.
struct Layout {
    uint64_t words;   // bitmap words, a whole number of tiles (>= one)
    size_t bm, pre, csum, icnt, total;
};

Layout layout(uint64_t n) {
    Layout l;
    const uint64_t tiles = n ? (n + kDelTile - 1) / kDelTile : 1;
    l.words = tiles * kDelWords;
    l.bm = kHdrBytes;
    l.pre = l.bm + l.words * 8;
    l.csum = l.pre + (((l.words + 1) * 4 + 15) & ~(size_t)15);
    l.icnt = l.csum + (size_t)kRankBlocks * 4;
    l.total = l.icnt + (size_t)kIdxBlocks * 4;
    return l;
}

// The fixed grids of the chunked passes: the word prefix over words + 1 entries
// (k_dml_word_sums, k_dml_word_prefix) and the index pass over n entries
// (k_dml_index_count, k_dml_index_write).
void prefix_chunks(uint64_t words, uint32_t* blocks, uint64_t* chunk) {
    chunks(words + 1, kTPB, kRankBlocks, blocks, chunk);
}

void index_chunks(uint64_t n, uint32_t* blocks, uint64_t* chunk) { chunks(n, kIdxStep, kIdxBlocks, blocks, chunk); }

// The plan last made by this thread: the apply steps take their sizes from it.
struct Plan {
    const void* ws;
    uint64_t n, deleted;
    int dev;
};
thread_local Plan g_plan = {nullptr, 0, 0, -1};

// The insert plan last made by this thread: n old rows, k new ones, n + k slots.
struct InsPlan {
    const void* ws;
    uint64_t n, k;
    int dev;
};
thread_local InsPlan g_iplan = {nullptr, 0, 0, -1};

__global__ __launch_bounds__(kTPB) void k_dml_mark(const int32_t* __restrict__ pos, uint64_t k, uint32_t n,
                                                   uint32_t* __restrict__ bm32, u64* __restrict__ bad) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    uint32_t nbad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x; i < k; i += stride) {
        const uint32_t p = (uint32_t)pos[i];  // a negative id is >= 2^31 > n
        if (p < n)
            atomicOr(bm32 + (p >> 5), 1u << (p & 31u));  // little-endian: bit p & 63 of u64 word p >> 6
        else
            nbad++;
    }
    const u64 wb = wave_sum_u64(nbad);
    if ((threadIdx.x & 63) == 0 && wb) atomicAdd(bad, wb);
}

// csum[b] = deleted rows in block b's chunk of `chunk` words; *deleted = their total.
__global__ __launch_bounds__(kTPB) void k_dml_word_sums(const u64* __restrict__ bm, uint64_t words, uint64_t chunk,
                                                        uint32_t* __restrict__ csum, u64* __restrict__ deleted) {
    __shared__ uint32_t s_w[kWaves];
    const uint64_t w0 = (uint64_t)blockIdx.x * chunk;
    const uint64_t w1 = w0 + chunk < words ? w0 + chunk : words;
    uint32_t c = 0;
    for (uint64_t w = w0 + threadIdx.x; w < w1; w += kTPB) c += (uint32_t)__popcll(bm[w]);
    const uint32_t total = block_sum(c, s_w);
    if (threadIdx.x == 0) {
        csum[blockIdx.x] = total;
        if (total) atomicAdd(deleted, (u64)total);
    }
}

// pre[w] = deleted rows before bitmap word w, for w in [0, words] (pre[words] = all).
__global__ __launch_bounds__(kTPB) void k_dml_word_prefix(const u64* __restrict__ bm, uint64_t words, uint64_t chunk,
                                                          const uint32_t* __restrict__ csum,
                                                          uint32_t* __restrict__ pre) {
    __shared__ uint32_t s_w[kWaves];
    uint32_t below = 0;
    for (uint32_t i = threadIdx.x; i < blockIdx.x; i += kTPB) below += csum[i];
    uint32_t base = block_sum(below, s_w);
    const uint64_t w0 = (uint64_t)blockIdx.x * chunk;
    const uint64_t w1 = w0 + chunk < words + 1 ? w0 + chunk : words + 1;
    for (uint64_t s = w0; s < w1; s += kTPB) {  // block-uniform trip count
        const uint64_t w = s + threadIdx.x;
        const uint32_t c = w < words ? (uint32_t)__popcll(bm[w]) : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_scan(c, s_w, &total);
        if (w < w1) pre[w] = base + ex;
        base += total;
    }
}

// The tile's rows in registers: lane t of step j holds rows j * 1024 + 4t .. + 3.
template <bool VEC>
__device__ __forceinline__ void load_tile(int4 (&v)[4], const int32_t* __restrict__ col, uint32_t rows, int tid) {
    if (rows == (uint32_t)kDelTile) {
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = load4_nt<VEC>(col + j * 1024 + tid * 4);
    } else {  // the column's last tile: one row at a time, none past the end
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t r = (uint32_t)(j * 1024 + tid * 4);
            v[j].x = r + 0 < rows ? col[r + 0] : 0;
            v[j].y = r + 1 < rows ? col[r + 1] : 0;
            v[j].z = r + 2 < rows ? col[r + 2] : 0;
            v[j].w = r + 3 < rows ? col[r + 3] : 0;
        }
    }
}

__global__ __launch_bounds__(kTPB) void k_dml_compact(ColPtrs cp, uint64_t n, const u64* __restrict__ bm,
                                                      const uint32_t* __restrict__ pre) {
    __shared__ __attribute__((aligned(16))) int s_buf[kDelTile + 4];
    __shared__ u64 s_word[kDelWords];
    __shared__ uint32_t s_pre[kDelWords + 1];
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * kDelTile;
    const uint64_t w0 = (uint64_t)blockIdx.x * kDelWords;
    if (tid < kDelWords) s_word[tid] = bm[w0 + tid];
    if (tid <= kDelWords) s_pre[tid] = pre[w0 + tid];
    __syncthreads();
    const uint32_t rows = n - t0 < (uint64_t)kDelTile ? (uint32_t)(n - t0) : (uint32_t)kDelTile;
    const uint32_t del0 = s_pre[0];
    const uint32_t cnt = rows - (s_pre[kDelWords] - del0);  // bits of rows >= n are never set
    if (cnt == 0) return;                                   // block-uniform
    const int32_t* __restrict__ col = cp.in[blockIdx.y] + t0;
    int32_t* __restrict__ out = cp.out[blockIdx.y] + (t0 - del0);  // the tile's first survivor
    const uint32_t a = (uint32_t)((reinterpret_cast<uintptr_t>(out) >> 2) & 3u);
    int4 v[4];
    if ((reinterpret_cast<uintptr_t>(cp.in[blockIdx.y]) & 15u) == 0)
        load_tile<true>(v, col, rows, tid);
    else
        load_tile<false>(v, col, rows, tid);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t lr = (uint32_t)(j * 1024 + tid * 4);  // the lane's 4 rows share one word
        const uint32_t wi = lr >> 6, bit = lr & 63u;
        const u64 w = s_word[wi];
        uint32_t k = a + lr - (s_pre[wi] - del0) - (uint32_t)__popcll(w & ((1ull << bit) - 1ull));
        const uint32_t nib = (uint32_t)(w >> bit) & 15u;
        if (!(nib & 1u) && lr + 0 < rows) s_buf[k++] = v[j].x;
        if (!(nib & 2u) && lr + 1 < rows) s_buf[k++] = v[j].y;
        if (!(nib & 4u) && lr + 2 < rows) s_buf[k++] = v[j].z;
        if (!(nib & 8u) && lr + 3 < rows) s_buf[k++] = v[j].w;
    }
    __syncthreads();
    const uint32_t end = a + cnt;
    int32_t* base = out - a;  // base + q is 16-byte aligned for q % 4 == 0
    for (uint32_t q = 4u * (uint32_t)tid; q < end; q += 4u * kTPB) {
        if (q >= a && q + 4u <= end) {
            *reinterpret_cast<int4*>(base + q) = *reinterpret_cast<const int4*>(s_buf + q);
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4; e++)
                if (q + e >= a && q + e < end) base[q + e] = s_buf[q + e];
        }
    }
}

// Deleted rows before row p, and whether p itself is deleted.
__device__ __forceinline__ uint32_t rank_of(const u64* __restrict__ bm, const uint32_t* __restrict__ pre, uint64_t p,
                                            bool* gone) {
    const u64 w = bm[p >> 6];
    const uint32_t bit = (uint32_t)p & 63u;
    *gone = (w >> bit) & 1ull;
    return pre[p >> 6] + (uint32_t)__popcll(w & ((1ull << bit) - 1ull));
}

// icnt[b] = surviving entries in block b's chunk of the index. A position outside
// [0, n) (not an index over these rows) counts as deleted: it is never looked up.
__global__ __launch_bounds__(kTPB) void k_dml_index_count(const u64* __restrict__ positions, uint64_t n, uint64_t chunk,
                                                          const u64* __restrict__ bm, uint32_t* __restrict__ icnt) {
    __shared__ uint32_t s_w[kWaves];
    const uint64_t i0 = (uint64_t)blockIdx.x * chunk;
    const uint64_t i1 = i0 + chunk < n ? i0 + chunk : n;
    uint32_t c = 0;
    for (uint64_t s = i0 + threadIdx.x; s < i1; s += kIdxStep) {
        u64 p[kIdxU];
#pragma unroll
        for (int u = 0; u < kIdxU; u++) p[u] = s + (uint64_t)u * kTPB < i1 ? positions[s + (uint64_t)u * kTPB] : ~0ull;
#pragma unroll
        for (int u = 0; u < kIdxU; u++)
            if (p[u] < n) c += !((bm[p[u] >> 6] >> (p[u] & 63ull)) & 1ull);
    }
    const uint32_t total = block_sum(c, s_w);
    if (threadIdx.x == 0) icnt[blockIdx.x] = total;
}

// The surviving entries of block b's chunk, in order, from the sum of the chunks below.
// Nothing is written at or past `cap` = n - deleted (positions that are no permutation
// of the rows could otherwise yield more survivors than the outputs hold).
__global__ __launch_bounds__(kTPB) void k_dml_index_write(const int32_t* __restrict__ values,
                                                          const u64* __restrict__ positions, uint64_t n, uint64_t chunk,
                                                          const u64* __restrict__ bm, const uint32_t* __restrict__ pre,
                                                          const uint32_t* __restrict__ icnt, uint64_t cap,
                                                          int32_t* __restrict__ values_out, u64* __restrict__ positions_out) {
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint32_t s_cnt[kIdxU][kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t below = 0;
    for (uint32_t i = threadIdx.x; i < blockIdx.x; i += kTPB) below += icnt[i];
    uint64_t base = block_sum(below, s_w);
    const uint64_t i0 = (uint64_t)blockIdx.x * chunk;
    const uint64_t i1 = i0 + chunk < n ? i0 + chunk : n;
    for (uint64_t s = i0; s < i1; s += kIdxStep) {  // block-uniform trip count
        u64 p[kIdxU];
        int32_t v[kIdxU];
        uint32_t rk[kIdxU];
        bool keep[kIdxU];
#pragma unroll
        for (int u = 0; u < kIdxU; u++) {
            const uint64_t i = s + (uint64_t)u * kTPB + threadIdx.x;
            p[u] = i < i1 ? positions[i] : ~0ull;
            v[u] = i < i1 ? values[i] : 0;
        }
#pragma unroll
        for (int u = 0; u < kIdxU; u++) {
            bool gone = true;
            rk[u] = p[u] < n ? rank_of(bm, pre, p[u], &gone) : 0u;
            keep[u] = !gone;
        }
        uint32_t in_wave[kIdxU];
        __syncthreads();  // the previous step's reads of s_cnt are done
#pragma unroll
        for (int u = 0; u < kIdxU; u++) {
            const u64 m = __ballot(keep[u]);
            in_wave[u] = lanes_below(m);
            if (lane == 0) s_cnt[u][wave] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        uint32_t run = 0;
#pragma unroll
        for (int u = 0; u < kIdxU; u++) {
            uint32_t mine = run;
#pragma unroll
            for (int w = 0; w < kWaves; w++) {
                const uint32_t c = s_cnt[u][w];
                mine += w < wave ? c : 0u;
                run += c;
            }
            const uint64_t o = base + mine + in_wave[u];
            if (keep[u] && o < cap) {
                if (values_out) values_out[o] = v[u];
                if (positions_out) positions_out[o] = p[u] - rk[u];
            }
        }
        base += run;
    }
}

__global__ __launch_bounds__(kTPB) void k_dml_update(int32_t* __restrict__ col, uint32_t n,
                                                     const int32_t* __restrict__ pos, uint64_t k, int32_t value,
                                                     u64* __restrict__ bad) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    uint32_t nbad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x; i < k; i += stride) {
        const uint32_t p = (uint32_t)pos[i];
        if (p < n)
            col[p] = value;
        else
            nbad++;
    }
    if (!bad) return;
    const u64 wb = wave_sum_u64(nbad);
    if ((threadIdx.x & 63) == 0 && wb) atomicAdd(bad, wb);
}

// ---- inserts ----

// Entries of the ascending a[0, n) that are <= v.
template <typename T, typename V>
__device__ __forceinline__ uint32_t upper_bound(const T* __restrict__ a, uint32_t n, V v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((V)a[mid] <= v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kTPB) void k_ins_points(const int32_t* __restrict__ sorted, uint32_t n,
                                                     const int32_t* __restrict__ nw, uint64_t k,
                                                     uint32_t* __restrict__ ins) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x; i < k; i += stride)
        ins[i] = upper_bound<int32_t, int32_t>(sorted, n, nw[i]);
}

// Slot ins[j] + j of the n + k output slots for the j-th new row. A point above n, or
// below the one before it, is counted and sets nothing, so no bit lies outside the map.
__global__ __launch_bounds__(kTPB) void k_ins_mark(const uint32_t* __restrict__ ins, uint64_t k, uint32_t n,
                                                   uint32_t* __restrict__ bm32, u64* __restrict__ bad) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    uint32_t nbad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x; i < k; i += stride) {
        const uint32_t p = ins[i];
        if (p <= n && (i == 0 || ins[i - 1] <= p)) {
            const uint64_t s = (uint64_t)p + i;  // < n + k < 2^31
            atomicOr(bm32 + (s >> 5), 1u << (s & 31u));
        } else {
            nbad++;
        }
    }
    const u64 wb = wave_sum_u64(nbad);
    if ((threadIdx.x & 63) == 0 && wb) atomicAdd(bad, wb);
}

// `count` <= kDelTile rows from src into LDS at s_dst[a + i], a = src's dword offset within
// its 16-byte line: every whole line is one nt dwordx4 load and one 16-byte LDS store,
// whatever the column's alignment; the ragged ends go row by row (none outside the
// range). All loads are issued before the first LDS store. s_dst is 16-byte aligned and
// receives zeros up to the end of the last line.
__device__ __forceinline__ uint32_t stage_rows(int* s_dst, const int32_t* __restrict__ src, uint32_t count, int tid) {
    const uint32_t a = (uint32_t)((reinterpret_cast<uintptr_t>(src) >> 2) & 3u);
    const int32_t* __restrict__ base = src - a;  // base + q is 16-byte aligned for q % 4 == 0
    const uint32_t end = a + count;              // <= kDelTile + 3: five steps of 1024
    int4 v[5];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const uint32_t q = (uint32_t)(j * 1024 + tid * 4);
        if (q >= a && q + 4u <= end) {
            v[j] = load4_nt<true>(base + q);
        } else {
            v[j].x = q + 0 >= a && q + 0 < end ? base[q + 0] : 0;
            v[j].y = q + 1 >= a && q + 1 < end ? base[q + 1] : 0;
            v[j].z = q + 2 >= a && q + 2 < end ? base[q + 2] : 0;
            v[j].w = q + 3 >= a && q + 3 < end ? base[q + 3] : 0;
        }
    }
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const uint32_t q = (uint32_t)(j * 1024 + tid * 4);
        if (q < end) *reinterpret_cast<int4*>(s_dst + q) = v[j];
    }
    return a;
}

// Output slots [t0, t0 + rows) of one column. ins0 new rows lie before the tile, so its
// old rows are old[t0 - ins0 ...) and its new rows new[ins0 ...), both contiguous.
__global__ __launch_bounds__(kTPB) void k_dml_expand(InsPtrs cp, uint64_t m, const u64* __restrict__ bm,
                                                     const uint32_t* __restrict__ pre) {
    __shared__ __attribute__((aligned(16))) int s_buf[kDelTile + 16];
    __shared__ u64 s_word[kDelWords];
    __shared__ uint32_t s_pre[kDelWords + 1];
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * kDelTile;
    const uint64_t w0 = (uint64_t)blockIdx.x * kDelWords;
    if (tid < kDelWords) s_word[tid] = bm[w0 + tid];
    if (tid <= kDelWords) s_pre[tid] = pre[w0 + tid];
    __syncthreads();
    const uint32_t rows = m - t0 < (uint64_t)kDelTile ? (uint32_t)(m - t0) : (uint32_t)kDelTile;
    const uint32_t ins0 = s_pre[0];
    const uint32_t cn = s_pre[kDelWords] - ins0;  // bits of slots >= m are never set
    const uint32_t co = rows - cn;
    // old rows at s_buf[ao + i], new rows behind them at s_buf[nb + an + i]:
    // nb + an + cn <= (co + 6) + 3 + cn <= kDelTile + 9
    uint32_t ao = 0, an = 0;
    if (co) ao = stage_rows(s_buf, cp.old_rows[blockIdx.y] + (t0 - ins0), co, tid);
    const uint32_t nb = (ao + co + 3u) & ~3u;
    if (cn) an = stage_rows(s_buf + nb, cp.new_rows[blockIdx.y] + ins0, cn, tid);
    __syncthreads();
    int32_t* __restrict__ out = cp.out[blockIdx.y] + t0;
    const bool vec = (reinterpret_cast<uintptr_t>(cp.out[blockIdx.y]) & 15u) == 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t lr = (uint32_t)(j * 1024 + tid * 4);  // the lane's 4 slots share one word
        if (lr >= rows) continue;
        const uint32_t wi = lr >> 6, bit = lr & 63u;
        const u64 w = s_word[wi];
        const uint32_t r1 = s_pre[wi] - ins0 + (uint32_t)__popcll(w & ((1ull << bit) - 1ull));
        const uint32_t nib = (uint32_t)(w >> bit) & 15u;
        uint32_t io = ao + lr - r1, in = nb + an + r1;  // both stay below kDelTile + 16
        int4 o;
        o.x = nib & 1u ? s_buf[in++] : s_buf[io++];
        o.y = nib & 2u ? s_buf[in++] : s_buf[io++];
        o.z = nib & 4u ? s_buf[in++] : s_buf[io++];
        o.w = nib & 8u ? s_buf[in++] : s_buf[io++];
        if (vec && lr + 4u <= rows) {
            *reinterpret_cast<int4*>(out + lr) = o;
        } else {
            if (lr + 0 < rows) out[lr + 0] = o.x;
            if (lr + 1 < rows) out[lr + 1] = o.y;
            if (lr + 2 < rows) out[lr + 2] = o.z;
            if (lr + 3 < rows) out[lr + 3] = o.w;
        }
    }
}

// The expansion over a sorted index: slot s takes the rank1(s)-th new entry or the
// (s - rank1(s))-th old one, whose position p moves up by the table's insertion points
// <= p when the table's rows were interleaved too (ren != NULL).
__global__ __launch_bounds__(kTPB) void k_ins_index(const int32_t* __restrict__ values, const u64* __restrict__ positions,
                                                    const int32_t* __restrict__ nvalues, const u64* __restrict__ npositions,
                                                    const uint32_t* __restrict__ ren, uint32_t kren, uint64_t m,
                                                    const u64* __restrict__ bm, const uint32_t* __restrict__ pre,
                                                    int32_t* __restrict__ values_out, u64* __restrict__ positions_out) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t s = (uint64_t)blockIdx.x * kTPB + threadIdx.x; s < m; s += stride) {
        const u64 w = bm[s >> 6];
        const uint32_t bit = (uint32_t)s & 63u;
        const uint32_t r1 = pre[s >> 6] + (uint32_t)__popcll(w & ((1ull << bit) - 1ull));
        int32_t v;
        u64 p;
        if ((w >> bit) & 1ull) {
            v = nvalues[r1];
            p = npositions[r1];
        } else {
            v = values[s - r1];
            p = positions[s - r1];
            if (ren) p += upper_bound<uint32_t, u64>(ren, kren, p);
        }
        values_out[s] = v;
        positions_out[s] = p;
    }
}

// slots[order ? order[j] : j] = ins[j] + j: the output slot of every new row, filed under
// its batch index. An order entry outside [0, k) files nothing.
__global__ __launch_bounds__(kTPB) void k_ins_slots(const uint32_t* __restrict__ ins, const u64* __restrict__ order,
                                                    uint64_t k, u64* __restrict__ slots) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x; i < k; i += stride) {
        const u64 o = order ? order[i] : i;
        if (o < k) slots[o] = (u64)ins[i] + i;
    }
}

// out[i] = the row of batch entry order[i]: its slot, or base + its batch index.
__global__ __launch_bounds__(kTPB) void k_ins_positions(const u64* __restrict__ slots, u64 base,
                                                        const u64* __restrict__ order, uint64_t k,
                                                        u64* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x; i < k; i += stride) {
        const u64 o = order[i];
        out[i] = o < k ? (slots ? slots[o] : base + o) : ~0ull;
    }
}

// The calling thread's plan on d_ws, or NULL.
const Plan* plan_on(const void* d_ws) {
    int dev = -1;
    if (!d_ws || g_plan.ws != d_ws || current_device(&dev) || dev != g_plan.dev) return nullptr;
    return &g_plan;
}

const InsPlan* insert_plan_on(const void* d_ws) {
    int dev = -1;
    if (!d_ws || g_iplan.ws != d_ws || current_device(&dev) || dev != g_iplan.dev) return nullptr;
    return &g_iplan;
}

}  // namespace

extern "C" {

size_t mq_delete_workspace_bytes(uint64_t n) { return layout(n).total; }

void mq_dml_geometry(uint64_t n, uint32_t* prefix_blocks, uint64_t* prefix_chunk_words, uint32_t* index_blocks,
                     uint64_t* index_chunk_rows) {
    uint32_t b;
    uint64_t c;
    prefix_chunks(layout(n).words, &b, &c);
    if (prefix_blocks) *prefix_blocks = b;
    if (prefix_chunk_words) *prefix_chunk_words = c;
    index_chunks(n, &b, &c);
    if (index_blocks) *index_blocks = b;
    if (index_chunk_rows) *index_chunk_rows = c;
}

int mq_delete_plan(const int32_t* d_pos, uint64_t k, uint64_t n, uint64_t* h_deleted, uint64_t* h_bad, void* d_ws,
                   size_t ws_bytes, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    g_plan.ws = nullptr;
    if (g_iplan.ws == d_ws) g_iplan.ws = nullptr;  // its bitmap is about to be overwritten
    if (!h_deleted || !h_bad || !d_ws || (k && !d_pos)) return set_err(MQ_EINVAL, "mq_delete_plan: NULL pointer");
    if (n >= (1ull << 31)) return set_err(MQ_EINVAL, "mq_delete_plan: n >= 2^31 (row ids are int32)");
    const Layout l = layout(n);
    if (ws_bytes < l.total) return set_err(MQ_EINVAL, "mq_delete_plan: workspace too small");
    if ((reinterpret_cast<uintptr_t>(d_ws) & 15u) != 0) return set_err(MQ_EINVAL, "mq_delete_plan: workspace not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(d_ws);
    u64* hdr = reinterpret_cast<u64*>(ws);
    u64* bm = reinterpret_cast<u64*>(ws + l.bm);
    uint32_t* pre = reinterpret_cast<uint32_t*>(ws + l.pre);
    uint32_t* csum = reinterpret_cast<uint32_t*>(ws + l.csum);
    HIPCHK(hipMemsetAsync(ws, 0, l.pre, st));  // the counters and the bitmap
    if (k) {
        hipLaunchKernelGGL(k_dml_mark, dim3(stream_grid(s, k)), dim3(kTPB), 0, st, d_pos, k, (uint32_t)n,
                           reinterpret_cast<uint32_t*>(bm), hdr);
        LAUNCHCHK("k_dml_mark");
    }
    uint32_t blocks;
    uint64_t chunk;
    prefix_chunks(l.words, &blocks, &chunk);
    hipLaunchKernelGGL(k_dml_word_sums, dim3(blocks), dim3(kTPB), 0, st, bm, l.words, chunk, csum, hdr + 1);
    LAUNCHCHK("k_dml_word_sums");
    hipLaunchKernelGGL(k_dml_word_prefix, dim3(blocks), dim3(kTPB), 0, st, bm, l.words, chunk, csum, pre);
    LAUNCHCHK("k_dml_word_prefix");
    uint64_t h[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h, hdr, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *h_bad = h[0];
    *h_deleted = h[1];
    if (h[0]) return set_err(MQ_EINVAL, "mq_delete_plan: %llu row ids outside [0, %llu)", (u64)h[0], (u64)n);
    int dev = -1;
    if ((rc = current_device(&dev))) return rc;
    g_plan = Plan{d_ws, n, h[1], dev};
    return MQ_OK;
}

int mq_delete_columns(const void* d_ws, const int32_t* const* d_cols, int ncols, int32_t* const* d_out, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    const Plan* pl = plan_on(d_ws);
    if (!pl) return set_err(MQ_EINVAL, "mq_delete_columns: no plan of this thread on this workspace");
    if (ncols < 0 || ncols > 1024) return set_err(MQ_EINVAL, "mq_delete_columns: ncols %d", ncols);
    if (ncols && (!d_cols || !d_out)) return set_err(MQ_EINVAL, "mq_delete_columns: NULL pointer");
    const uint64_t n = pl->n, left = n - pl->deleted;
    for (int j = 0; j < ncols; j++) {
        if (n && !d_cols[j]) return set_err(MQ_EINVAL, "mq_delete_columns: NULL column %d", j);
        if (left && !d_out[j]) return set_err(MQ_EINVAL, "mq_delete_columns: NULL output %d", j);
        if (left && d_out[j] == d_cols[j]) return set_err(MQ_EINVAL, "mq_delete_columns: column %d in place", j);
        if ((reinterpret_cast<uintptr_t>(d_cols[j]) & 3u) || (reinterpret_cast<uintptr_t>(d_out[j]) & 3u))
            return set_err(MQ_EINVAL, "mq_delete_columns: column %d not 4-byte aligned", j);
    }
    if (left == 0 || ncols == 0) return MQ_OK;
    const Layout l = layout(n);
    const char* ws = static_cast<const char*>(d_ws);
    const u64* bm = reinterpret_cast<const u64*>(ws + l.bm);
    const uint32_t* pre = reinterpret_cast<const uint32_t*>(ws + l.pre);
    const uint32_t tiles = (uint32_t)((n + kDelTile - 1) / kDelTile);
    for (int j0 = 0; j0 < ncols; j0 += kColsPerLaunch) {
        const int c = ncols - j0 < kColsPerLaunch ? ncols - j0 : kColsPerLaunch;
        ColPtrs cp = {};
        for (int j = 0; j < c; j++) {
            cp.in[j] = d_cols[j0 + j];
            cp.out[j] = d_out[j0 + j];
        }
        hipLaunchKernelGGL(k_dml_compact, dim3(tiles, (uint32_t)c), dim3(kTPB), 0, (hipStream_t)stream, cp, n, bm, pre);
        LAUNCHCHK("k_dml_compact");
    }
    return MQ_OK;
}

int mq_delete_index(void* d_ws, const int32_t* d_values, const uint64_t* d_positions, int32_t* d_values_out,
                    uint64_t* d_positions_out, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    const Plan* pl = plan_on(d_ws);
    if (!pl) return set_err(MQ_EINVAL, "mq_delete_index: no plan of this thread on this workspace");
    const uint64_t n = pl->n, left = n - pl->deleted;
    if (n && (!d_values || !d_positions)) return set_err(MQ_EINVAL, "mq_delete_index: NULL pointer");
    if (left && (!d_values_out || !d_positions_out)) return set_err(MQ_EINVAL, "mq_delete_index: NULL output");
    if (left && (d_values_out == d_values || d_positions_out == d_positions))
        return set_err(MQ_EINVAL, "mq_delete_index: in place");
    if (left == 0) return MQ_OK;
    const Layout l = layout(n);
    char* ws = static_cast<char*>(d_ws);
    const u64* bm = reinterpret_cast<const u64*>(ws + l.bm);
    const uint32_t* pre = reinterpret_cast<const uint32_t*>(ws + l.pre);
    uint32_t* icnt = reinterpret_cast<uint32_t*>(ws + l.icnt);
    const u64* pos = reinterpret_cast<const u64*>(d_positions);
    hipStream_t st = (hipStream_t)stream;
    uint32_t blocks;
    uint64_t chunk;
    index_chunks(n, &blocks, &chunk);
    hipLaunchKernelGGL(k_dml_index_count, dim3(blocks), dim3(kTPB), 0, st, pos, n, chunk, bm, icnt);
    LAUNCHCHK("k_dml_index_count");
    hipLaunchKernelGGL(k_dml_index_write, dim3(blocks), dim3(kTPB), 0, st, d_values, pos, n, chunk, bm, pre, icnt, left,
                       d_values_out, reinterpret_cast<u64*>(d_positions_out));
    LAUNCHCHK("k_dml_index_write");
    return MQ_OK;
}

size_t mq_insert_workspace_bytes(uint64_t n, uint64_t k) { return layout(n + k).total; }

int mq_insert_points(const int32_t* d_sorted, uint64_t n, const int32_t* d_new_sorted, uint64_t k, uint32_t* d_ins,
                     void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if ((n && !d_sorted) || (k && (!d_new_sorted || !d_ins))) return set_err(MQ_EINVAL, "mq_insert_points: NULL pointer");
    if (n + k >= (1ull << 31) || n + k < n) return set_err(MQ_EINVAL, "mq_insert_points: n + k >= 2^31 (row ids are int32)");
    if (k == 0) return MQ_OK;
    hipLaunchKernelGGL(k_ins_points, dim3(stream_grid(s, k)), dim3(kTPB), 0, (hipStream_t)stream, d_sorted, (uint32_t)n,
                       d_new_sorted, k, d_ins);
    LAUNCHCHK("k_ins_points");
    return MQ_OK;
}

int mq_insert_plan(const uint32_t* d_ins, uint64_t k, uint64_t n, uint64_t* h_bad, void* d_ws, size_t ws_bytes,
                   void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    g_iplan.ws = nullptr;
    if (g_plan.ws == d_ws) g_plan.ws = nullptr;  // its bitmap is about to be overwritten
    if (!h_bad || !d_ws || (k && !d_ins)) return set_err(MQ_EINVAL, "mq_insert_plan: NULL pointer");
    if (n + k >= (1ull << 31) || n + k < n) return set_err(MQ_EINVAL, "mq_insert_plan: n + k >= 2^31 (row ids are int32)");
    const Layout l = layout(n + k);
    if (ws_bytes < l.total) return set_err(MQ_EINVAL, "mq_insert_plan: workspace too small");
    if ((reinterpret_cast<uintptr_t>(d_ws) & 15u) != 0) return set_err(MQ_EINVAL, "mq_insert_plan: workspace not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(d_ws);
    u64* hdr = reinterpret_cast<u64*>(ws);
    u64* bm = reinterpret_cast<u64*>(ws + l.bm);
    uint32_t* pre = reinterpret_cast<uint32_t*>(ws + l.pre);
    uint32_t* csum = reinterpret_cast<uint32_t*>(ws + l.csum);
    HIPCHK(hipMemsetAsync(ws, 0, l.pre, st));  // the counters and the bitmap
    if (k) {
        hipLaunchKernelGGL(k_ins_mark, dim3(stream_grid(s, k)), dim3(kTPB), 0, st, d_ins, k, (uint32_t)n,
                           reinterpret_cast<uint32_t*>(bm), hdr);
        LAUNCHCHK("k_ins_mark");
    }
    uint32_t blocks;
    uint64_t chunk;
    prefix_chunks(l.words, &blocks, &chunk);
    hipLaunchKernelGGL(k_dml_word_sums, dim3(blocks), dim3(kTPB), 0, st, bm, l.words, chunk, csum, hdr + 1);
    LAUNCHCHK("k_dml_word_sums");
    hipLaunchKernelGGL(k_dml_word_prefix, dim3(blocks), dim3(kTPB), 0, st, bm, l.words, chunk, csum, pre);
    LAUNCHCHK("k_dml_word_prefix");
    uint64_t h[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h, hdr, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *h_bad = h[0];
    if (h[0])
        return set_err(MQ_EINVAL, "mq_insert_plan: %llu insertion points descend or exceed %llu", (u64)h[0], (u64)n);
    if (h[1] != k) return set_err(MQ_EHIP, "mq_insert_plan: %llu slots marked for %llu rows", (u64)h[1], (u64)k);
    int dev = -1;
    if ((rc = current_device(&dev))) return rc;
    g_iplan = InsPlan{d_ws, n, k, dev};
    return MQ_OK;
}

int mq_insert_columns(const void* d_ws, const int32_t* const* d_old, const int32_t* const* d_new, int ncols,
                      int32_t* const* d_out, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    const InsPlan* pl = insert_plan_on(d_ws);
    if (!pl) return set_err(MQ_EINVAL, "mq_insert_columns: no plan of this thread on this workspace");
    if (ncols < 0 || ncols > 1024) return set_err(MQ_EINVAL, "mq_insert_columns: ncols %d", ncols);
    if (ncols && (!d_old || !d_new || !d_out)) return set_err(MQ_EINVAL, "mq_insert_columns: NULL pointer");
    const uint64_t n = pl->n, k = pl->k, m = n + k;
    for (int j = 0; j < ncols; j++) {
        if ((n && !d_old[j]) || (k && !d_new[j]) || (m && !d_out[j]))
            return set_err(MQ_EINVAL, "mq_insert_columns: NULL column %d", j);
        if (m && (d_out[j] == d_old[j] || d_out[j] == d_new[j]))
            return set_err(MQ_EINVAL, "mq_insert_columns: column %d in place", j);
        if ((reinterpret_cast<uintptr_t>(d_old[j]) & 3u) || (reinterpret_cast<uintptr_t>(d_new[j]) & 3u) ||
            (reinterpret_cast<uintptr_t>(d_out[j]) & 3u))
            return set_err(MQ_EINVAL, "mq_insert_columns: column %d not 4-byte aligned", j);
    }
    if (m == 0 || ncols == 0) return MQ_OK;
    const Layout l = layout(m);
    const char* ws = static_cast<const char*>(d_ws);
    const u64* bm = reinterpret_cast<const u64*>(ws + l.bm);
    const uint32_t* pre = reinterpret_cast<const uint32_t*>(ws + l.pre);
    const uint32_t tiles = (uint32_t)((m + kDelTile - 1) / kDelTile);
    for (int j0 = 0; j0 < ncols; j0 += kColsPerLaunch) {
        const int c = ncols - j0 < kColsPerLaunch ? ncols - j0 : kColsPerLaunch;
        InsPtrs cp = {};
        for (int j = 0; j < c; j++) {
            cp.old_rows[j] = d_old[j0 + j];
            cp.new_rows[j] = d_new[j0 + j];
            cp.out[j] = d_out[j0 + j];
        }
        hipLaunchKernelGGL(k_dml_expand, dim3(tiles, (uint32_t)c), dim3(kTPB), 0, (hipStream_t)stream, cp, m, bm, pre);
        LAUNCHCHK("k_dml_expand");
    }
    return MQ_OK;
}

int mq_insert_index(const void* d_ws, const int32_t* d_values, const uint64_t* d_positions, const int32_t* d_new_values,
                    const uint64_t* d_new_positions, const uint32_t* d_renumber_ins, uint64_t k_renumber,
                    int32_t* d_values_out, uint64_t* d_positions_out, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    const InsPlan* pl = insert_plan_on(d_ws);
    if (!pl) return set_err(MQ_EINVAL, "mq_insert_index: no plan of this thread on this workspace");
    const uint64_t n = pl->n, k = pl->k, m = n + k;
    if ((n && (!d_values || !d_positions)) || (k && (!d_new_values || !d_new_positions)))
        return set_err(MQ_EINVAL, "mq_insert_index: NULL pointer");
    if (m && (!d_values_out || !d_positions_out)) return set_err(MQ_EINVAL, "mq_insert_index: NULL output");
    if (m && (d_values_out == d_values || d_positions_out == d_positions))
        return set_err(MQ_EINVAL, "mq_insert_index: in place");
    if (k_renumber >= (1ull << 31)) return set_err(MQ_EINVAL, "mq_insert_index: k_renumber >= 2^31");
    if (m == 0) return MQ_OK;
    const Layout l = layout(m);
    const char* ws = static_cast<const char*>(d_ws);
    hipLaunchKernelGGL(k_ins_index, dim3(stream_grid(s, m)), dim3(kTPB), 0, (hipStream_t)stream, d_values,
                       reinterpret_cast<const u64*>(d_positions), d_new_values, reinterpret_cast<const u64*>(d_new_positions),
                       k_renumber ? d_renumber_ins : nullptr, (uint32_t)k_renumber, m, reinterpret_cast<const u64*>(ws + l.bm),
                       reinterpret_cast<const uint32_t*>(ws + l.pre), d_values_out, reinterpret_cast<u64*>(d_positions_out));
    LAUNCHCHK("k_ins_index");
    return MQ_OK;
}

int mq_insert_slots(const uint32_t* d_ins, const uint64_t* d_order, uint64_t k, uint64_t* d_slots, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (k && (!d_ins || !d_slots)) return set_err(MQ_EINVAL, "mq_insert_slots: NULL pointer");
    if (k >= (1ull << 31)) return set_err(MQ_EINVAL, "mq_insert_slots: k >= 2^31");
    if (k == 0) return MQ_OK;
    hipLaunchKernelGGL(k_ins_slots, dim3(stream_grid(s, k)), dim3(kTPB), 0, (hipStream_t)stream, d_ins,
                       reinterpret_cast<const u64*>(d_order), k, reinterpret_cast<u64*>(d_slots));
    LAUNCHCHK("k_ins_slots");
    return MQ_OK;
}

int mq_insert_positions(const uint64_t* d_slots, uint64_t base, const uint64_t* d_order, uint64_t k, uint64_t* d_out,
                        void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (k && (!d_order || !d_out)) return set_err(MQ_EINVAL, "mq_insert_positions: NULL pointer");
    if (k >= (1ull << 31)) return set_err(MQ_EINVAL, "mq_insert_positions: k >= 2^31");
    if (k == 0) return MQ_OK;
    hipLaunchKernelGGL(k_ins_positions, dim3(stream_grid(s, k)), dim3(kTPB), 0, (hipStream_t)stream,
                       reinterpret_cast<const u64*>(d_slots), (u64)base, reinterpret_cast<const u64*>(d_order), k,
                       reinterpret_cast<u64*>(d_out));
    LAUNCHCHK("k_ins_positions");
    return MQ_OK;
}

int mq_update_rows(int32_t* d_col, uint64_t n, const int32_t* d_pos, uint64_t k, int32_t value, uint64_t* d_bad,
                   void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if ((n && !d_col) || (k && !d_pos)) return set_err(MQ_EINVAL, "mq_update_rows: NULL pointer");
    if (n >= (1ull << 31)) return set_err(MQ_EINVAL, "mq_update_rows: n >= 2^31 (row ids are int32)");
    hipStream_t st = (hipStream_t)stream;
    if (d_bad) HIPCHK(hipMemsetAsync(d_bad, 0, sizeof(uint64_t), st));
    if (k == 0) return MQ_OK;
    hipLaunchKernelGGL(k_dml_update, dim3(stream_grid(s, k)), dim3(kTPB), 0, st, d_col, (uint32_t)n, d_pos, k, value,
                       reinterpret_cast<u64*>(d_bad));
    LAUNCHCHK("k_dml_update");
    return MQ_OK;
}

}  // extern "C"
