// mq_topk64.hip — HAVING, ORDER BY and LIMIT over int64 entries: the first k passing entries of a
// stable sort, as (value, index).
//
// n entries v[i] (int64; NULL: the order is i itself) and an optional filter column h[i] with a
// range (entry i passes when low <= h[i] < high) give the first m = min(k, passed) passing entries
// of a stable sort by v, ascending or descending, equal values in ascending i either way. The
// reference has no such operator; the semantics are restated in numpy by tests/topk64cases.py.
// The result is unique, so every path, grid and candidate cap gives the same bytes.
//
// An entry's order is that of the u64 key (uint64)v ^ 2^63, complemented for descending
// (mq_topk64_key): the key ascends in output order. mq_topk.hip (§3.12) is the 32-bit model of
// this unit; its kernels are not shared, the structure is.
//
// select (k far below n), levels + 1 streaming reads:
//   k_topk64_hist   : contiguous chunks, 4 entries a lane a tile as two 16-byte loads, kU tiles in
//                     flight. With a filter column the filter is read first and the value only for
//                     a wave tile (256 entries) in which an entry passed. Counts a digit of the key
//                     (11 bits at shifts 53, 42, 31, 20, 9, then the last 9) over the passing
//                     entries whose higher digits equal the boundary's, into a table in LDS. A wave
//                     tile that falls into one bin whole is counted in a scalar and the run of such
//                     tiles flushed with one update. The table leaves with plain stores to the
//                     block's own slice of the scratch.
//   k_topk64_fold   : per bin, the sum over the blocks' tables; the host walks the sums to the bin
//                     B that holds the m-th key. The first level's total is `passed`.
//   k_topk64_pick   : per block, its entries in bins below B (added over the levels) and in B.
//   k_topk64_scan   : one block, the exclusive prefixes of those two counts over the blocks.
//   k_topk64_collect: the same chunks again. A passing entry before the boundary prefix is emitted;
//                     one on it while its rank among such entries is below `take`: all of them when
//                     they fit the candidate cap, else (a single value by then) the first m - below.
//                     Output slot = entries-before-the-prefix before it + min(rank, take): index
//                     order. Emits (key, index).
//   then a stable sort of the candidates by key, as two mq_index_build runs (the low word, then the
//   high word through the first run's positions), and k_topk64_gather of the first m.
//
// sort (ORDER BY without a useful LIMIT): one counting read (every passing entry into one bin),
// the same collect with take = passed, the same sort of all of them.
//
// no values (HAVING and LIMIT in index order): the counting read, the collect with take = m; the
// candidates are the result.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "mq_common.h"
#include "mq_device.h"
#include "mq_group_impl.h"
#include "mq_scan_common.h"

namespace {

using namespace mqi;
using u64 = unsigned long long;
using i64 = long long;

constexpr uint32_t kBins = 2048;              // the widest digit: 8 KiB of LDS a block
constexpr int kU = 2;                         // tiles in flight per thread (64 B a column a lane)
constexpr int kFoldBins = 16;                 // bins per fold workgroup
constexpr int kFoldParts = kTPB / kFoldBins;  // block strides per bin
constexpr uint64_t kMaxCap = 1ull << 31;
constexpr u64 kSign = 1ull << 63;

struct Level {
    int shift;
    uint32_t bins;
};
constexpr int kNumLevels = 6;
constexpr Level kLevels[kNumLevels] = {{53, 2048}, {42, 2048}, {31, 2048}, {20, 2048}, {9, 2048}, {0, 512}};

// h passes when (u64)h - lo <= wm1: one compare for low <= h < high (the host folds missing bounds
// and empty ranges; see make_pred64).
struct Pred64 {
    u64 lo;
    u64 wm1;
};

// The filter of a call: 0 none, 1 on a column of its own, 2 on the value column itself.
enum { kNoFilter = 0, kFilterCol = 1, kFilterVals = 2 };

typedef i64 v2l __attribute__((ext_vector_type(2)));

template <bool VEC>
__device__ __forceinline__ void load4x64(const i64* __restrict__ p, i64 (&v)[4]) {
    if constexpr (VEC) {
        const v2l a = __builtin_nontemporal_load(reinterpret_cast<const v2l*>(p));
        const v2l b = __builtin_nontemporal_load(reinterpret_cast<const v2l*>(p + 2));
        v[0] = a.x;
        v[1] = a.y;
        v[2] = b.x;
        v[3] = b.y;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = __builtin_nontemporal_load(p + e);
    }
}

__device__ __forceinline__ bool passes(i64 h, Pred64 pr) { return (u64)h - pr.lo <= pr.wm1; }

// One full tile's four entries of this lane: p[e] = entry e passes, v[e] = its value (0 where the
// values are not wanted, or not read because no entry of the wave's 256 passed).
template <bool VEC, int FILT>
__device__ __forceinline__ void load_tile(const i64* __restrict__ vals, const i64* __restrict__ hav, Pred64 pr, uint64_t row,
                                          bool want_vals, i64 (&v)[4], bool (&p)[4]) {
#pragma unroll
    for (int e = 0; e < 4; e++) {
        v[e] = 0;
        p[e] = true;
    }
    if constexpr (FILT == kFilterCol) {
        i64 h[4];
        load4x64<VEC>(hav + row, h);
#pragma unroll
        for (int e = 0; e < 4; e++) p[e] = passes(h[e], pr);
        if (want_vals && __any(p[0] || p[1] || p[2] || p[3])) load4x64<VEC>(vals + row, v);  // wave-uniform
    } else {
        if (want_vals || FILT == kFilterVals) load4x64<VEC>(vals + row, v);
        if constexpr (FILT == kFilterVals) {
#pragma unroll
            for (int e = 0; e < 4; e++) p[e] = passes(v[e], pr);
        }
    }
}

// The same for the chunk's ragged last tile: entry by entry, none past `end`.
template <int FILT>
__device__ __forceinline__ void load_ragged(const i64* __restrict__ vals, const i64* __restrict__ hav, Pred64 pr, uint64_t row,
                                            uint64_t end, bool want_vals, i64 (&v)[4], bool (&p)[4]) {
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const bool ok = row + e < end;
        v[e] = 0;
        p[e] = ok;
        if (!ok) continue;
        if constexpr (FILT == kFilterCol) {
            p[e] = passes(hav[row + e], pr);
            if (p[e] && want_vals) v[e] = vals[row + e];
        } else {
            if (want_vals || FILT == kFilterVals) v[e] = vals[row + e];
            if constexpr (FILT == kFilterVals) p[e] = passes(v[e], pr);
        }
    }
}

// want_vals == 0 (with mask == 0 and bmask == 0): a counting read, every passing entry into bin 0.
template <bool VEC, int FILT>
__global__ __launch_bounds__(kTPB, 8) void k_topk64_hist(const i64* __restrict__ vals, const i64* __restrict__ hav, Pred64 pr,
                                                         uint64_t n, uint64_t rows_per_block, u64 flip, u64 mask, u64 pfx,
                                                         int shift, uint32_t bins, int want_vals, uint32_t* __restrict__ tabs) {
    __shared__ uint32_t s_cnt[kBins];
    const int tid = threadIdx.x, lane = tid & 63;
    for (uint32_t b = tid; b < bins; b += kTPB) s_cnt[b] = 0u;
    __syncthreads();
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;
    const uint32_t bmask = bins - 1;

    // the wave's run of tiles whose 256 entries all pass and fall into run_bin (wave-uniform)
    uint32_t run_bin = 0, run_rows = 0;

    auto flush = [&]() {
        if (lane == 0) atomicAdd(&s_cnt[run_bin], run_rows);
        run_rows = 0;
    };
    auto consume = [&](const i64(&v)[4], const bool(&p)[4], bool full) {
        bool in[4];
        uint32_t b[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const u64 key = (u64)v[e] ^ flip;
            in[e] = p[e] && (key & mask) == pfx;
            b[e] = (uint32_t)(key >> shift) & bmask;
        }
        const uint32_t first = __builtin_amdgcn_readfirstlane(b[0]);
        if (full && __all(in[0] && in[1] && in[2] && in[3] && b[0] == first && b[1] == first && b[2] == first && b[3] == first)) {
            if (run_rows && first != run_bin) flush();
            run_bin = first;
            run_rows += 256u;
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (in[e]) atomicAdd(&s_cnt[b[e]], 1u);
        }
    };

    uint64_t t = start;
    for (; t + (uint64_t)kU * kTileRows <= end; t += (uint64_t)kU * kTileRows) {
        i64 v[kU][4];
        bool p[kU][4];
#pragma unroll
        for (int u = 0; u < kU; u++)
            load_tile<VEC, FILT>(vals, hav, pr, t + (uint64_t)u * kTileRows + (uint64_t)tid * 4, want_vals != 0, v[u], p[u]);
#pragma unroll
        for (int u = 0; u < kU; u++) consume(v[u], p[u], true);
    }
    for (; t < end; t += kTileRows) {  // the chunk's tail
        const uint64_t row = t + (uint64_t)tid * 4;
        i64 v[4];
        bool p[4];
        if (t + kTileRows <= end) {  // block-uniform
            load_tile<VEC, FILT>(vals, hav, pr, row, want_vals != 0, v, p);
            consume(v, p, true);
        } else {
            load_ragged<FILT>(vals, hav, pr, row, end, want_vals != 0, v, p);
            consume(v, p, false);
        }
    }
    if (run_rows) flush();
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * bins;
    for (uint32_t b = tid; b < bins; b += kTPB) tabs[base + b] = s_cnt[b];
}

// counts[b] = the sum of the blocks' tables at bin b.
__global__ __launch_bounds__(kTPB) void k_topk64_fold(const uint32_t* __restrict__ tabs, uint32_t blocks, uint32_t bins,
                                                      u64* __restrict__ counts) {
    __shared__ u64 p_cnt[kFoldParts][kFoldBins];
    const uint32_t sl = threadIdx.x % kFoldBins, part = threadIdx.x / kFoldBins;
    const uint32_t b = blockIdx.x * kFoldBins + sl;
    u64 c = 0;
    if (b < bins)
        for (uint32_t k = part; k < blocks; k += kFoldParts) c += tabs[(size_t)k * bins + b];
    p_cnt[part][sl] = c;
    __syncthreads();
    if (part == 0 && b < bins) {
        for (int p = 1; p < kFoldParts; p++) c += p_cnt[p][sl];
        counts[b] = c;
    }
}

// One wave per block table: blk_below[k] (+)= its entries in bins below B, blk_in[k] = those in B.
__global__ __launch_bounds__(kTPB) void k_topk64_pick(const uint32_t* __restrict__ tabs, uint32_t blocks, uint32_t bins,
                                                      uint32_t B, int first, uint32_t* __restrict__ blk_below,
                                                      uint32_t* __restrict__ blk_in) {
    const uint32_t k = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= blocks) return;  // wave-uniform
    const uint32_t* tab = tabs + (size_t)k * bins;
    u64 c = 0;
    for (uint32_t b = lane; b < B; b += 64) c += tab[b];
    c = wave_sum_u64(c);
    if (lane == 0) {
        blk_below[k] = (first ? 0u : blk_below[k]) + (uint32_t)c;
        blk_in[k] = tab[B];
    }
}

// One block: both arrays become their exclusive prefixes over the blocks (sums below 2^31).
__global__ __launch_bounds__(kTPB) void k_topk64_scan(uint32_t* __restrict__ blk_below, uint32_t* __restrict__ blk_in,
                                                      uint32_t blocks) {
    __shared__ uint32_t s_w[kWaves];
    uint32_t run_b = 0, run_t = 0;
    for (uint32_t k0 = 0; k0 < blocks; k0 += kTPB) {  // block-uniform trip count
        const uint32_t k = k0 + threadIdx.x;
        const uint32_t vb = k < blocks ? blk_below[k] : 0u, vt = k < blocks ? blk_in[k] : 0u;
        uint32_t tb, tt;
        const uint32_t eb = block_excl_scan(vb, s_w, &tb);
        const uint32_t et = block_excl_scan(vt, s_w, &tt);
        if (k < blocks) {
            blk_below[k] = run_b + eb;
            blk_in[k] = run_t + et;
        }
        run_b += tb;
        run_t += tt;
    }
}

// vals == NULL: the key of entry i is i (mask and pfx are 0 then: every passing entry is on the prefix).
template <bool VEC, int FILT>
__global__ __launch_bounds__(kTPB) void k_topk64_collect(const i64* __restrict__ vals, const i64* __restrict__ hav, Pred64 pr,
                                                         uint64_t n, uint64_t rows_per_block, u64 flip, u64 mask, u64 pfx,
                                                         uint32_t take, const uint32_t* __restrict__ off_below,
                                                         const uint32_t* __restrict__ off_in, uint32_t cand,
                                                         u64* __restrict__ c_key, uint32_t* __restrict__ c_idx) {
    __shared__ uint32_t s_w[kWaves];
    const int tid = threadIdx.x;
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;
    const bool want_vals = vals != nullptr;
    // entries before the prefix, and entries on it, ahead of the tile (block-uniform)
    uint32_t nb_run = off_below[blockIdx.x], nt_run = off_in[blockIdx.x];

    // an entry's class: 1 before the boundary prefix, 2 on it, 0 behind it or filtered out
    auto cls = [&](i64 v, bool p) {
        const u64 km = ((u64)v ^ flip) & mask;
        return !p ? 0u : km < pfx ? 1u : km == pfx ? 2u : 0u;
    };
    auto emit = [&](uint32_t o, i64 v, uint64_t row) {
        if (o >= cand) return;  // never: the counts come from the same entries
        c_key[o] = want_vals ? (u64)v ^ flip : (u64)row;
        c_idx[o] = (uint32_t)row;
    };
    // one tile whose entries' classes are c[0..3]; block-uniform call
    auto place = [&](const i64(&v)[4], const uint32_t(&c)[4], uint64_t row) {
        uint32_t cb = 0, ct = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            cb += c[e] == 1u;
            ct += c[e] == 2u;
        }
        uint32_t total;
        const uint32_t ex = block_excl_scan(cb | (ct << 16), s_w, &total);  // each sum <= 1024
        uint32_t lb = nb_run + (ex & 0xffffu), lt = nt_run + (ex >> 16);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (c[e] == 1u) {
                emit(lb + (lt < take ? lt : take), v[e], row + e);
                lb++;
            } else if (c[e] == 2u) {
                if (lt < take) emit(lb + lt, v[e], row + e);
                lt++;
            }
        }
        nb_run += total & 0xffffu;
        nt_run += total >> 16;
    };

    uint64_t t = start;
    for (; t + (uint64_t)kU * kTileRows <= end; t += (uint64_t)kU * kTileRows) {
        i64 v[kU][4];
        uint32_t c[kU][4];
        bool any = false;
#pragma unroll
        for (int u = 0; u < kU; u++) {
            bool p[4];
            load_tile<VEC, FILT>(vals, hav, pr, t + (uint64_t)u * kTileRows + (uint64_t)tid * 4, want_vals, v[u], p);
#pragma unroll
            for (int e = 0; e < 4; e++) {
                c[u][e] = cls(v[u][e], p[e]);
                any |= c[u][e] == 1u || (c[u][e] == 2u && nt_run < take);
            }
        }
        // Nothing to emit in the group: no entry before the prefix, and the entries on it, if any,
        // are all past `take` already (nt_run only grows, so it need not be kept up then).
        if (!__syncthreads_or(any)) continue;
#pragma unroll
        for (int u = 0; u < kU; u++) place(v[u], c[u], t + (uint64_t)u * kTileRows + (uint64_t)tid * 4);
    }
    for (; t < end; t += kTileRows) {  // the chunk's tail, the ragged last tile included
        const uint64_t row = t + (uint64_t)tid * 4;
        i64 v[4];
        bool p[4];
        uint32_t c[4];
        load_ragged<FILT>(vals, hav, pr, row, end, want_vals, v, p);
#pragma unroll
        for (int e = 0; e < 4; e++) c[e] = cls(v[e], p[e]);
        place(v, c, row);
    }
}

// out[i] = a word of the candidates' keys as the int32 that mq_index_build orders the same way:
// the low word (pos == NULL), or the high word of candidate pos[i].
__global__ __launch_bounds__(kTPB) void k_topk64_word(const u64* __restrict__ c_key, const u64* __restrict__ pos, uint32_t count,
                                                      int32_t* __restrict__ out) {
    const uint32_t stride = gridDim.x * kTPB;
    for (uint32_t i = blockIdx.x * kTPB + threadIdx.x; i < count; i += stride) {
        u64 w;
        if (pos) {
            const u64 p = pos[i];
            w = (p < count ? c_key[p] : 0ull) >> 32;  // always p < count: a permutation of [0, count)
        } else {
            w = c_key[i];
        }
        out[i] = (int32_t)((uint32_t)w ^ 0x80000000u);
    }
}

// The candidate behind sorted entry i: pos1[pos2[i]], or i itself when the candidates are in order.
__device__ __forceinline__ uint32_t sorted_cand(const u64* __restrict__ pos1, const u64* __restrict__ pos2, uint32_t i,
                                                uint32_t count) {
    if (!pos2) return i;
    const u64 a = pos2[i];
    const u64 b = a < count ? pos1[a] : 0ull;
    return b < count ? (uint32_t)b : 0u;  // always in range: permutations of [0, count)
}

// The first m sorted entries: the value back from its key, the index of the entry.
__global__ __launch_bounds__(kTPB) void k_topk64_gather(const u64* __restrict__ c_key, const uint32_t* __restrict__ c_idx,
                                                        const u64* __restrict__ pos1, const u64* __restrict__ pos2, uint32_t m,
                                                        uint32_t count, u64 vflip, i64* __restrict__ vals_out,
                                                        uint32_t* __restrict__ idx_out) {
    const uint32_t i = blockIdx.x * kTPB + threadIdx.x;
    if (i >= m) return;
    const uint32_t c = sorted_cand(pos1, pos2, i, count);
    if (vals_out) vals_out[i] = (i64)(c_key[c] ^ vflip);
    if (idx_out) idx_out[i] = c_idx[c];
}

// *out = sorted entries at or past m whose key equals entry m - 1's: a binary search.
__global__ void k_topk64_ties(const u64* __restrict__ c_key, const u64* __restrict__ pos1, const u64* __restrict__ pos2,
                              uint32_t count, uint32_t m, u64* __restrict__ out) {
    if (threadIdx.x || blockIdx.x) return;
    const u64 T = c_key[sorted_cand(pos1, pos2, m - 1, count)];
    uint32_t lo = m, hi = count;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (c_key[sorted_cand(pos1, pos2, mid, count)] == T) lo = mid + 1;
        else hi = mid;
    }
    *out = lo - m;
}

// out[i] = in[i], sign-extended.
__global__ __launch_bounds__(kTPB) void k_topk64_widen(const int32_t* __restrict__ in, uint64_t n, i64* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x; i < n; i += stride) out[i] = in[i];
}

// out[i] = col[idx[i]], elements of 4 or 8 bytes.
template <typename T>
__global__ __launch_bounds__(kTPB) void k_topk64_take(const T* __restrict__ col, const uint32_t* __restrict__ idx, uint64_t m,
                                                      T* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x; i < m; i += stride) out[i] = col[idx[i]];
}

// The call's device buffers: freed once the stream has drained, on every way out.
struct Scratch {
    static constexpr int kMax = 16;
    void* p[kMax];
    int used = 0;
    hipStream_t st;
    explicit Scratch(hipStream_t s) : st(s) {}
    void* get(size_t bytes) {
        if (used == kMax) return nullptr;
        void* q = pool_alloc(bytes ? bytes : 16);
        if (q) p[used++] = q;
        return q;
    }
    ~Scratch() {
        if (used) (void)hipStreamSynchronize(st);
        for (int i = 0; i < used; i++) pool_free(p[i]);
    }
};

// Folds the bounds into one unsigned compare; false: no int64 passes.
bool make_pred64(const mq_range64* r, Pred64* p) {
    const int64_t lo = r->has_low ? r->low : INT64_MIN;
    if (r->has_high && r->high == INT64_MIN) return false;
    const int64_t hi = r->has_high ? r->high - 1 : INT64_MAX;  // inclusive
    if (hi < lo) return false;
    p->lo = (u64)lo;
    p->wm1 = (u64)hi - (u64)lo;
    return true;
}

struct Call {
    const DevState* s;
    const i64* vals;
    const i64* hav;
    Pred64 pr;
    int filt;
    bool vec;
    uint64_t n;
    u64 flip;
    uint32_t g;
    uint64_t rpb;
    hipStream_t st;
};

template <bool VEC, int FILT>
const void* hist_fn() {
    return reinterpret_cast<const void*>(&k_topk64_hist<VEC, FILT>);
}
const void* hist_fn_of(const Call& c) {
    if (c.vec) return c.filt == kNoFilter ? hist_fn<true, kNoFilter>() : c.filt == kFilterCol ? hist_fn<true, kFilterCol>() : hist_fn<true, kFilterVals>();
    return c.filt == kNoFilter ? hist_fn<false, kNoFilter>() : c.filt == kFilterCol ? hist_fn<false, kFilterCol>() : hist_fn<false, kFilterVals>();
}

template <bool VEC, int FILT>
void launch_hist_as(const Call& c, u64 mask, u64 pfx, int shift, uint32_t bins, int want_vals, uint32_t* tabs) {
    hipLaunchKernelGGL((k_topk64_hist<VEC, FILT>), dim3(c.g), dim3(kTPB), 0, c.st, c.vals, c.hav, c.pr, c.n, c.rpb, c.flip, mask,
                       pfx, shift, bins, want_vals, tabs);
}
void launch_hist(const Call& c, u64 mask, u64 pfx, int shift, uint32_t bins, int want_vals, uint32_t* tabs) {
    if (c.vec) {
        if (c.filt == kNoFilter) launch_hist_as<true, kNoFilter>(c, mask, pfx, shift, bins, want_vals, tabs);
        else if (c.filt == kFilterCol) launch_hist_as<true, kFilterCol>(c, mask, pfx, shift, bins, want_vals, tabs);
        else launch_hist_as<true, kFilterVals>(c, mask, pfx, shift, bins, want_vals, tabs);
    } else {
        if (c.filt == kNoFilter) launch_hist_as<false, kNoFilter>(c, mask, pfx, shift, bins, want_vals, tabs);
        else if (c.filt == kFilterCol) launch_hist_as<false, kFilterCol>(c, mask, pfx, shift, bins, want_vals, tabs);
        else launch_hist_as<false, kFilterVals>(c, mask, pfx, shift, bins, want_vals, tabs);
    }
}

template <bool VEC, int FILT>
void launch_collect_as(const Call& c, u64 mask, u64 pfx, uint32_t take, const uint32_t* off_below, const uint32_t* off_in,
                       uint32_t cand, u64* c_key, uint32_t* c_idx) {
    hipLaunchKernelGGL((k_topk64_collect<VEC, FILT>), dim3(c.g), dim3(kTPB), 0, c.st, c.vals, c.hav, c.pr, c.n, c.rpb, c.flip,
                       mask, pfx, take, off_below, off_in, cand, c_key, c_idx);
}
void launch_collect(const Call& c, u64 mask, u64 pfx, uint32_t take, const uint32_t* off_below, const uint32_t* off_in,
                    uint32_t cand, u64* c_key, uint32_t* c_idx) {
    if (c.vec) {
        if (c.filt == kNoFilter) launch_collect_as<true, kNoFilter>(c, mask, pfx, take, off_below, off_in, cand, c_key, c_idx);
        else if (c.filt == kFilterCol) launch_collect_as<true, kFilterCol>(c, mask, pfx, take, off_below, off_in, cand, c_key, c_idx);
        else launch_collect_as<true, kFilterVals>(c, mask, pfx, take, off_below, off_in, cand, c_key, c_idx);
    } else {
        if (c.filt == kNoFilter) launch_collect_as<false, kNoFilter>(c, mask, pfx, take, off_below, off_in, cand, c_key, c_idx);
        else if (c.filt == kFilterCol) launch_collect_as<false, kFilterCol>(c, mask, pfx, take, off_below, off_in, cand, c_key, c_idx);
        else launch_collect_as<false, kFilterVals>(c, mask, pfx, take, off_below, off_in, cand, c_key, c_idx);
    }
}

// Sorts `count` candidates by key (stable; sorted == true: they are in order already), writes the
// first m entries and, when asked, the number of entries past m whose key equals the m-th.
int finish(const DevState* s, Scratch& sc, const u64* c_key, const uint32_t* c_idx, uint64_t count, bool sorted, uint64_t m,
           u64 vflip, int64_t* vals_out, uint32_t* idx_out, uint64_t* ties, hipStream_t st) {
    u64 *pos1 = nullptr, *pos2 = nullptr;
    if (!sorted) {
        int32_t* word = static_cast<int32_t*>(sc.get(count * 4));
        pos1 = static_cast<u64*>(sc.get(count * 8));
        pos2 = static_cast<u64*>(sc.get(count * 8));
        if (!word || !pos1 || !pos2) return set_err(MQ_ENOMEM, "mq_topk64: sort buffers allocation failed");
        const uint32_t grid = stream_grid(s, count);
        hipLaunchKernelGGL(k_topk64_word, dim3(grid), dim3(kTPB), 0, st, c_key, (const u64*)nullptr, (uint32_t)count, word);
        LAUNCHCHK("k_topk64_word");
        int rc = mq_index_build(word, count, nullptr, reinterpret_cast<uint64_t*>(pos1), st);  // synchronises
        if (rc) return rc;
        hipLaunchKernelGGL(k_topk64_word, dim3(grid), dim3(kTPB), 0, st, c_key, (const u64*)pos1, (uint32_t)count, word);
        LAUNCHCHK("k_topk64_word");
        rc = mq_index_build(word, count, nullptr, reinterpret_cast<uint64_t*>(pos2), st);
        if (rc) return rc;
    }
    if (vals_out || idx_out) {
        hipLaunchKernelGGL(k_topk64_gather, dim3((uint32_t)((m + kTPB - 1) / kTPB)), dim3(kTPB), 0, st, c_key, c_idx,
                           (const u64*)pos1, (const u64*)pos2, (uint32_t)m, (uint32_t)count, vflip,
                           reinterpret_cast<i64*>(vals_out), idx_out);
        LAUNCHCHK("k_topk64_gather");
    }
    if (ties) {
        u64* d_ties = static_cast<u64*>(sc.get(8));
        if (!d_ties) return set_err(MQ_ENOMEM, "mq_topk64: allocation failed");
        hipLaunchKernelGGL(k_topk64_ties, dim3(1), dim3(64), 0, st, c_key, (const u64*)pos1, (const u64*)pos2, (uint32_t)count,
                           (uint32_t)m, d_ties);
        LAUNCHCHK("k_topk64_ties");
        u64 h = 0;
        HIPCHK(hipMemcpyAsync(&h, d_ties, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        *ties = h;
    }
    HIPCHK(hipStreamSynchronize(st));
    return MQ_OK;
}

int topk64_run(Call& c, uint64_t k, bool select, uint64_t cap, int64_t* vals_out, uint32_t* idx_out, mq_topk64_info* info) {
    hipStream_t st = c.st;
    Scratch sc(st);
    geometry(c.s, c.n, hist_fn_of(c), &c.g, &c.rpb, (uint64_t)kU * kTileRows);
    const uint32_t g = c.g;
    const bool ordered = c.vals != nullptr;  // else the order is the index: no boundary to find
    const bool asked_select = select;
    if (!ordered || k == 0) select = false;
    uint32_t* tabs = static_cast<uint32_t*>(sc.get((size_t)g * (select ? kBins : 1) * 4));
    u64* counts = static_cast<u64*>(sc.get(kBins * 8));
    uint32_t* blk = static_cast<uint32_t*>(sc.get((size_t)g * 8));
    if (!tabs || !counts || !blk) return set_err(MQ_ENOMEM, "mq_topk64: scratch allocation failed");
    uint32_t *blk_below = blk, *blk_in = blk + g;

    static thread_local u64 hc[kBins];
    u64 mask = 0, pfx = 0;
    uint64_t below = 0, in_bin = 0, passed = 0, m = 0;
    int levels = 0;
    const int nlev = select ? kNumLevels : 1;
    for (int L = 0; L < nlev; L++) {
        // without a boundary to find: a counting read, every passing entry into one bin
        const int shift = select ? kLevels[L].shift : 0;
        const uint32_t bins = select ? kLevels[L].bins : 1u;
        launch_hist(c, mask, pfx, shift, bins, select ? 1 : 0, tabs);
        LAUNCHCHK("k_topk64_hist");
        hipLaunchKernelGGL(k_topk64_fold, dim3((bins + kFoldBins - 1) / kFoldBins), dim3(kTPB), 0, st, tabs, g, bins, counts);
        LAUNCHCHK("k_topk64_fold");
        HIPCHK(hipMemcpyAsync(hc, counts, (size_t)bins * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (L == 0) {
            for (uint32_t b = 0; b < bins; b++) passed += hc[b];
            m = k < passed ? k : passed;
            if (info) {
                info->passed = passed;
                info->m = m;
            }
            if (m == 0) return MQ_OK;
        }
        // the bin that holds the m-th key: `need` more entries are wanted from this prefix
        const uint64_t need = select ? m - below : 1;
        uint64_t acc = 0;
        uint32_t B = bins;
        for (uint32_t b = 0; b < bins; b++) {
            if (acc + hc[b] >= need) {
                B = b;
                break;
            }
            acc += hc[b];
        }
        if (B == bins) return set_err(MQ_EHIP, "mq_topk64: level %d counted %llu entries, %llu wanted", L, (u64)acc, (u64)need);
        below += acc;
        in_bin = hc[B];
        hipLaunchKernelGGL(k_topk64_pick, dim3((g + kWaves - 1) / kWaves), dim3(kTPB), 0, st, tabs, g, bins, B, L == 0, blk_below,
                           blk_in);
        LAUNCHCHK("k_topk64_pick");
        if (select) {
            pfx |= (u64)B << shift;
            mask |= (u64)(bins - 1) << shift;
            levels = L + 1;
            if (in_bin <= cap) break;
        }
    }
    // Entries on the boundary prefix. select: all of them when they fit the cap, else (six levels:
    // the prefix is one value) the first r in index order. sort: every passing entry. No values:
    // the first m passing entries.
    const uint64_t r = m - below;  // select: 1 .. in_bin
    const bool all = !select ? ordered : in_bin <= cap;
    const uint64_t take = all ? in_bin : r;
    const uint64_t cand = below + take;  // <= passed
    hipLaunchKernelGGL(k_topk64_scan, dim3(1), dim3(kTPB), 0, st, blk_below, blk_in, g);
    LAUNCHCHK("k_topk64_scan");
    u64* c_key = static_cast<u64*>(sc.get(cand * 8));
    uint32_t* c_idx = static_cast<uint32_t*>(sc.get(cand * 4));
    if (!c_key || !c_idx) return set_err(MQ_ENOMEM, "mq_topk64: candidate buffers allocation failed");
    launch_collect(c, mask, pfx, (uint32_t)take, blk_below, blk_in, (uint32_t)cand, c_key, c_idx);
    LAUNCHCHK("k_topk64_collect");
    uint64_t ties = 0;
    const int rc = finish(c.s, sc, c_key, c_idx, cand, !ordered, m, ordered ? c.flip : 0ull, vals_out, idx_out,
                          info && ordered && all ? &ties : nullptr, st);
    if (rc) return rc;
    if (info) {
        info->candidates = cand;
        info->ties = !ordered ? 0 : all ? ties : in_bin - r;
        info->levels = ordered ? levels : asked_select ? 1 : 0;  // the counting read
    }
    return MQ_OK;
}

}  // namespace

// What mq_group.hip's mq_group_top shares (mq_group_impl.h): the kernels stay this unit's own.
namespace mqi {

void topk64_launch_widen(const int32_t* in, uint64_t n, int64_t* out, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(k_topk64_widen, dim3(grid), dim3(kTPB), 0, st, in, n, reinterpret_cast<i64*>(out));
}

void topk64_launch_take32(const int32_t* col, const uint32_t* idx, uint64_t m, int32_t* out, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL((k_topk64_take<int32_t>), dim3(grid), dim3(kTPB), 0, st, col, idx, m, out);
}

void topk64_launch_take64(const int64_t* col, const uint32_t* idx, uint64_t m, int64_t* out, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL((k_topk64_take<i64>), dim3(grid), dim3(kTPB), 0, st, reinterpret_cast<const i64*>(col), idx, m,
                       reinterpret_cast<i64*>(out));
}

}  // namespace mqi

extern "C" {

uint64_t mq_topk64_key(int64_t v, int descending) { return ((uint64_t)v ^ kSign) ^ (descending ? ~0ull : 0ull); }

int mq_topk64_auto_path(uint64_t n, uint64_t k, uint64_t cand_cap) {
    const uint64_t m = k < n ? k : n;
    uint64_t cap = cand_cap ? cand_cap : mq_topk_default_cap();
    if (cap > kMaxCap) cap = kMaxCap;
    return m + cap > n / MQ_TOPK_SORT_DIV ? MQ_TOPK_SORT : MQ_TOPK_SELECT;
}

int mq_topk64(const int64_t* d_vals, const int64_t* d_having, const mq_range64* h_having, uint64_t n, uint64_t k, int descending,
              int path, uint64_t cand_cap, int64_t* d_vals_out, uint32_t* d_idx_out, mq_topk64_info* h_info, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (h_info) memset(h_info, 0, sizeof *h_info);
    if (path != MQ_TOPK_AUTO && path != MQ_TOPK_SELECT && path != MQ_TOPK_SORT)
        return set_err(MQ_EINVAL, "mq_topk64: path %d", path);
    if (n >= (1ull << 31)) return set_err(MQ_EINVAL, "mq_topk64: n >= 2^31");
    if ((reinterpret_cast<uintptr_t>(d_vals) & 7u) || (reinterpret_cast<uintptr_t>(d_having) & 7u) ||
        (reinterpret_cast<uintptr_t>(d_vals_out) & 7u))
        return set_err(MQ_EINVAL, "mq_topk64: column not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_idx_out) & 3u) return set_err(MQ_EINVAL, "mq_topk64: indices not 4-byte aligned");
    if (d_having && !h_having) return set_err(MQ_EINVAL, "mq_topk64: a filter column without a range");
    uint64_t cap = cand_cap ? cand_cap : mq_topk_default_cap();
    if (cap > kMaxCap) cap = kMaxCap;
    const int taken = path != MQ_TOPK_AUTO ? path : mq_topk64_auto_path(n, k, cap);
    if (h_info) h_info->path = taken;
    Call c = {};
    c.s = s;
    c.vals = reinterpret_cast<const i64*>(d_vals);
    c.hav = reinterpret_cast<const i64*>(d_having);
    c.filt = !d_having ? kNoFilter : d_having == d_vals ? kFilterVals : kFilterCol;
    if (d_having && !make_pred64(h_having, &c.pr)) return MQ_OK;  // no int64 passes: nothing is read
    if (n == 0 || k == 0) {
        if (h_info && k == 0 && n && !d_having) h_info->passed = n;
        if (n == 0 || !h_info || !d_having) return MQ_OK;
        // k == 0 under a filter: the info still reports the passing entries (one counting read)
    }
    c.vec = aligned16(d_vals) && aligned16(d_having);
    c.n = n;
    c.flip = kSign ^ (descending ? ~0ull : 0ull);
    c.st = (hipStream_t)stream;
    return topk64_run(c, k, taken == MQ_TOPK_SELECT, cap, d_vals_out, d_idx_out, h_info);
}

int mq_topk64_widen(const int32_t* d_in, uint64_t n, int64_t* d_out, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (n && (!d_in || !d_out)) return set_err(MQ_EINVAL, "mq_topk64_widen: NULL pointer");
    if ((reinterpret_cast<uintptr_t>(d_in) & 3u) || (reinterpret_cast<uintptr_t>(d_out) & 7u))
        return set_err(MQ_EINVAL, "mq_topk64_widen: misaligned pointer");
    if (n == 0) return MQ_OK;
    topk64_launch_widen(d_in, n, d_out, stream_grid(s, n), (hipStream_t)stream);
    LAUNCHCHK("k_topk64_widen");
    return MQ_OK;
}

int mq_topk64_take(const void* d_col, int elem_bytes, const uint32_t* d_idx, uint64_t m, void* d_out, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (elem_bytes != 4 && elem_bytes != 8) return set_err(MQ_EINVAL, "mq_topk64_take: elements of %d bytes", elem_bytes);
    if (m && (!d_col || !d_idx || !d_out)) return set_err(MQ_EINVAL, "mq_topk64_take: NULL pointer");
    const uintptr_t am = (uintptr_t)elem_bytes - 1;
    if ((reinterpret_cast<uintptr_t>(d_col) & am) || (reinterpret_cast<uintptr_t>(d_out) & am) ||
        (reinterpret_cast<uintptr_t>(d_idx) & 3u))
        return set_err(MQ_EINVAL, "mq_topk64_take: misaligned pointer");
    if (m == 0) return MQ_OK;
    const uint32_t grid = stream_grid(s, m);
    if (elem_bytes == 4)
        topk64_launch_take32(static_cast<const int32_t*>(d_col), d_idx, m, static_cast<int32_t*>(d_out), grid, (hipStream_t)stream);
    else
        topk64_launch_take64(static_cast<const int64_t*>(d_col), d_idx, m, static_cast<int64_t*>(d_out), grid, (hipStream_t)stream);
    LAUNCHCHK("k_topk64_take");
    return MQ_OK;
}

}  // extern "C"
