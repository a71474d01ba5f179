// mq_topk.hip — the k smallest or largest rows of an int32 column, in order.
//
// n rows v[i] with an optional payload p[i] (p[i] = i without one) give the first
// m = min(k, n) entries of a stable sort of the rows: ascending by v, or descending by v,
// equal values in ascending row order either way. The reference has no such operator; the
// semantics are restated in numpy by tests/topkcases.py. The result is unique, so every
// path and grid gives the same bytes.
//
// A row's order is that of the u32 key (uint32)v ^ 2^31, complemented for descending: the
// key ascends in output order, and key ^ 2^31 (v, or ~v for descending) is the int32 the
// project's one sort, mq_index_build, orders the same way.
//
// select (k far below n), levels + 1 streaming reads of the column:
//   k_topk_hist   : k_scan's chunking and nt dwordx4 loads, kTopU tiles in flight. Counts a
//                   digit of the key (its top 11 bits, then the next 11, then the last 10) over
//                   the rows whose higher digits equal the boundary's, into a table in LDS with
//                   LDS atomics. A wave tile (256 rows) that falls into one bin is counted in a
//                   scalar instead and the run of such tiles flushed with one update: a
//                   low-cardinality column issues a handful of atomics per block. The block's
//                   table leaves with plain stores to its own slice of the scratch.
//   k_topk_fold   : per bin, the sum over the blocks' tables. The host reads the 2048 sums
//                   and walks them to the bin B that holds the m-th key.
//   k_topk_pick   : per block, its rows in bins below B (added over the levels) and in B:
//                   what the collect pass needs to place a block's output, so the column is
//                   not read again to count.
//   k_topk_scan   : one block, the exclusive prefixes of those two counts over the blocks.
//   k_topk_collect: the same chunks again. A row before the boundary prefix is emitted; a row
//                   on it is emitted while its rank among such rows (the blocks before, then
//                   the rows before it in the block) is below `take`: all of them when they
//                   fit the candidate cap, else (a single value T by then) the first
//                   r = m - below. Output slot = rows-before-the-prefix before it +
//                   min(rank, take): input order. Groups of tiles in which no row can be
//                   emitted cost one barrier.
//   then mq_index_build of the candidates' keys (stable: ties stay in input order) and
//   k_topk_gather of the first m through its positions.
//
// sort (k so large that selecting saves nothing): mq_index_build of the whole column (of ~v
// for descending), k_topk_gather of the first m.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "mq_common.h"
#include "mq_device.h"
#include "mq_scan_common.h"

namespace {

using namespace mqi;
using u64 = unsigned long long;

constexpr uint32_t kBins = 2048;              // the widest digit: 8 KiB of LDS a block
constexpr int kTopU = 4;                      // tiles in flight per thread
constexpr int kFoldBins = 16;                 // bins per fold workgroup
constexpr int kFoldParts = kTPB / kFoldBins;  // block strides per bin
constexpr uint64_t kDefaultCap = 1ull << 20;
constexpr uint64_t kMaxCap = 1ull << 31;

struct Level {
    int shift;
    uint32_t bins;
};
constexpr Level kLevels[3] = {{21, 2048}, {10, 2048}, {0, 1024}};

template <bool VEC>
__global__ __launch_bounds__(kTPB, 8) void k_topk_hist(const int* __restrict__ col, uint64_t n, uint64_t rows_per_block,
                                                       uint32_t flip, uint32_t mask, uint32_t pfx, int shift, uint32_t bins,
                                                       uint32_t* __restrict__ tabs) {
    __shared__ uint32_t s_cnt[kBins];
    const int tid = threadIdx.x, lane = tid & 63;
    for (uint32_t b = tid; b < bins; b += kTPB) s_cnt[b] = 0u;
    __syncthreads();
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;
    const uint32_t bmask = bins - 1;

    // the wave's run of tiles whose 256 rows all fall into run_bin (wave-uniform)
    uint32_t run_bin = 0, run_rows = 0;

    auto update = [&](int v) {
        const uint32_t key = (uint32_t)v ^ flip;
        if ((key & mask) == pfx) atomicAdd(&s_cnt[(key >> shift) & bmask], 1u);
    };
    auto flush = [&]() {
        if (lane == 0) atomicAdd(&s_cnt[run_bin], run_rows);
        run_rows = 0;
    };
    auto consume = [&](int4 v) {  // a full tile
        const uint32_t k0 = (uint32_t)v.x ^ flip, k1 = (uint32_t)v.y ^ flip, k2 = (uint32_t)v.z ^ flip,
                       k3 = (uint32_t)v.w ^ flip;
        const bool in0 = (k0 & mask) == pfx, in1 = (k1 & mask) == pfx, in2 = (k2 & mask) == pfx, in3 = (k3 & mask) == pfx;
        const uint32_t b0 = (k0 >> shift) & bmask, b1 = (k1 >> shift) & bmask, b2 = (k2 >> shift) & bmask,
                       b3 = (k3 >> shift) & bmask;
        const uint32_t first = __builtin_amdgcn_readfirstlane(b0);
        if (__all(in0 && in1 && in2 && in3 && b0 == first && b1 == first && b2 == first && b3 == first)) {
            if (run_rows && first != run_bin) flush();
            run_bin = first;
            run_rows += 256u;
        } else if (__any(in0 || in1 || in2 || in3)) {
            if (in0) atomicAdd(&s_cnt[b0], 1u);
            if (in1) atomicAdd(&s_cnt[b1], 1u);
            if (in2) atomicAdd(&s_cnt[b2], 1u);
            if (in3) atomicAdd(&s_cnt[b3], 1u);
        }
    };

    uint64_t t = start;
    for (; t + (uint64_t)kTopU * kTileRows <= end; t += (uint64_t)kTopU * kTileRows) {
        int4 v[kTopU];
#pragma unroll
        for (int u = 0; u < kTopU; u++) v[u] = load4_nt<VEC>(col + t + (uint64_t)u * kTileRows + (uint64_t)tid * 4);
#pragma unroll
        for (int u = 0; u < kTopU; u++) consume(v[u]);
    }
    for (; t < end; t += kTileRows) {  // the chunk's tail
        const uint64_t row = t + (uint64_t)tid * 4;
        if (t + kTileRows <= end) {    // block-uniform
            consume(load4_nt<VEC>(col + row));
        } else {                       // the last ragged tile: row by row, none past the end
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (row + e < end) update(col[row + e]);
        }
    }
    if (run_rows) flush();
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * bins;
    for (uint32_t b = tid; b < bins; b += kTPB) tabs[base + b] = s_cnt[b];
}

// counts[b] = the sum of the blocks' tables at bin b.
__global__ __launch_bounds__(kTPB) void k_topk_fold(const uint32_t* __restrict__ tabs, uint32_t blocks, uint32_t bins,
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

// One wave per block table: blk_below[k] (+)= its rows in bins below B, blk_in[k] = its rows in B.
__global__ __launch_bounds__(kTPB) void k_topk_pick(const uint32_t* __restrict__ tabs, uint32_t blocks, uint32_t bins,
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
__global__ __launch_bounds__(kTPB) void k_topk_scan(uint32_t* __restrict__ blk_below, uint32_t* __restrict__ blk_in,
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

template <bool VEC>
__global__ __launch_bounds__(kTPB) void k_topk_collect(const int* __restrict__ col, const int* __restrict__ payload,
                                                       uint64_t n, uint64_t rows_per_block, uint32_t flip, uint32_t mask,
                                                       uint32_t pfx, uint32_t take, const uint32_t* __restrict__ off_below,
                                                       const uint32_t* __restrict__ off_in, uint32_t cand,
                                                       int32_t* __restrict__ c_key, int32_t* __restrict__ c_pay) {
    __shared__ uint32_t s_w[kWaves];
    const int tid = threadIdx.x;
    const uint64_t start = (uint64_t)blockIdx.x * rows_per_block;
    uint64_t end = start + rows_per_block;
    if (end > n) end = n;
    // rows before the prefix, and rows on it, ahead of the tile (block-uniform)
    uint32_t nb_run = off_below[blockIdx.x], nt_run = off_in[blockIdx.x];

    // a row's class: 1 before the boundary prefix, 2 on it, 0 behind it
    auto cls = [&](int v) {
        const uint32_t km = ((uint32_t)v ^ flip) & mask;
        return km < pfx ? 1u : km == pfx ? 2u : 0u;
    };
    auto emit = [&](uint32_t o, int v, uint64_t row) {
        if (o >= cand) return;  // never: the counts come from the same rows
        c_key[o] = (int32_t)((uint32_t)v ^ flip ^ 0x80000000u);
        c_pay[o] = payload ? payload[row] : (int32_t)row;
    };
    // one tile whose rows' classes are c[0..3]; block-uniform call
    auto place = [&](const int* v, const uint32_t* c, uint64_t row) {
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
    for (; t + (uint64_t)kTopU * kTileRows <= end; t += (uint64_t)kTopU * kTileRows) {
        int4 q[kTopU];
#pragma unroll
        for (int u = 0; u < kTopU; u++) q[u] = load4_nt<VEC>(col + t + (uint64_t)u * kTileRows + (uint64_t)tid * 4);
        uint32_t c[kTopU][4];
        bool any = false;
#pragma unroll
        for (int u = 0; u < kTopU; u++) {
            c[u][0] = cls(q[u].x);
            c[u][1] = cls(q[u].y);
            c[u][2] = cls(q[u].z);
            c[u][3] = cls(q[u].w);
#pragma unroll
            for (int e = 0; e < 4; e++) any |= c[u][e] == 1u || (c[u][e] == 2u && nt_run < take);
        }
        // Nothing to emit in the group: no row before the prefix, and the rows on it, if any,
        // are all past `take` already (nt_run only grows, so it need not be kept up then).
        if (!__syncthreads_or(any)) continue;
#pragma unroll
        for (int u = 0; u < kTopU; u++) {
            const int v[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
            place(v, c[u], t + (uint64_t)u * kTileRows + (uint64_t)tid * 4);
        }
    }
    for (; t < end; t += kTileRows) {  // the chunk's tail, the ragged last tile included
        const uint64_t row = t + (uint64_t)tid * 4;
        int v[4];
        uint32_t c[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const bool ok = row + e < end;
            v[e] = ok ? col[row + e] : 0;
            c[e] = ok ? cls(v[e]) : 0u;
        }
        place(v, c, row);
    }
}

// out[i] = ~in[i]: the descending sort path's keys.
__global__ __launch_bounds__(kTPB) void k_topk_not(const int32_t* __restrict__ in, uint64_t n, int32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x; i < n; i += stride) out[i] = ~in[i];
}

// The first m sorted entries: the value back from its key, the payload through the position.
__global__ __launch_bounds__(kTPB) void k_topk_gather(const int32_t* __restrict__ sorted, const u64* __restrict__ pos,
                                                      const int32_t* __restrict__ pay, uint32_t m, uint32_t count,
                                                      uint32_t vflip, int32_t* __restrict__ vals_out,
                                                      int32_t* __restrict__ pay_out) {
    const uint32_t i = blockIdx.x * kTPB + threadIdx.x;
    if (i >= m) return;
    if (vals_out) vals_out[i] = (int32_t)((uint32_t)sorted[i] ^ vflip);
    if (pay_out) {
        const u64 p = pos[i];
        if (p < count) pay_out[i] = pay ? pay[p] : (int32_t)p;  // always: a permutation of [0, count)
    }
}

// *out = entries at or past m that equal entry m - 1 (sorted ascending): a binary search.
__global__ void k_topk_ties(const int32_t* __restrict__ sorted, uint32_t count, uint32_t m, u64* __restrict__ out) {
    if (threadIdx.x || blockIdx.x) return;
    const int32_t T = sorted[m - 1];
    uint32_t lo = m, hi = count;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (sorted[mid] == T) lo = mid + 1;
        else hi = mid;
    }
    *out = lo - m;
}

// The call's device buffers: freed once the stream has drained, on every way out.
struct Scratch {
    void* p[10];
    int used = 0;
    hipStream_t st;
    explicit Scratch(hipStream_t s) : st(s) {}
    void* get(size_t bytes) {
        if (used == 10) return nullptr;
        void* q = pool_alloc(bytes ? bytes : 16);
        if (q) p[used++] = q;
        return q;
    }
    ~Scratch() {
        if (used) (void)hipStreamSynchronize(st);
        for (int i = 0; i < used; i++) pool_free(p[i]);
    }
};

// Sorts `count` keys (stable), writes the first m entries and, when asked, the number of
// entries past m that equal the m-th. pay: per key, or NULL for the key's own index.
int finish(Scratch& sc, const int32_t* keys, uint64_t count, const int32_t* pay, uint64_t m, uint32_t vflip,
           int32_t* vals_out, int32_t* pay_out, uint64_t* ties, hipStream_t st) {
    int32_t* sorted = static_cast<int32_t*>(sc.get(count * 4));
    u64* pos = static_cast<u64*>(sc.get(count * 8));
    u64* d_ties = static_cast<u64*>(sc.get(8));
    if (!sorted || !pos || !d_ties) return set_err(MQ_ENOMEM, "mq_topk: sort buffers allocation failed");
    int rc = mq_index_build(keys, count, sorted, reinterpret_cast<uint64_t*>(pos), st);  // synchronises
    if (rc) return rc;
    if (vals_out || pay_out) {
        hipLaunchKernelGGL(k_topk_gather, dim3((uint32_t)((m + kTPB - 1) / kTPB)), dim3(kTPB), 0, st, sorted, pos, pay,
                           (uint32_t)m, (uint32_t)count, vflip, vals_out, pay_out);
        LAUNCHCHK("k_topk_gather");
    }
    if (ties) {
        hipLaunchKernelGGL(k_topk_ties, dim3(1), dim3(64), 0, st, sorted, (uint32_t)count, (uint32_t)m, d_ties);
        LAUNCHCHK("k_topk_ties");
        u64 h = 0;
        HIPCHK(hipMemcpyAsync(&h, d_ties, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        *ties = h;
    }
    HIPCHK(hipStreamSynchronize(st));
    return MQ_OK;
}

int topk_sort(const DevState* s, const int32_t* vals, const int32_t* payload, uint64_t n, uint64_t m, int desc,
              int32_t* vals_out, int32_t* pay_out, mq_topk_info* info, hipStream_t st) {
    Scratch sc(st);
    const int32_t* keys = vals;
    if (desc) {
        int32_t* inv = static_cast<int32_t*>(sc.get(n * 4));
        if (!inv) return set_err(MQ_ENOMEM, "mq_topk: key buffer allocation failed");
        hipLaunchKernelGGL(k_topk_not, dim3(stream_grid(s, n)), dim3(kTPB), 0, st, vals, n, inv);
        LAUNCHCHK("k_topk_not");
        keys = inv;
    }
    uint64_t ties = 0;
    const int rc = finish(sc, keys, n, payload, m, desc ? ~0u : 0u, vals_out, pay_out, info ? &ties : nullptr, st);
    if (rc) return rc;
    if (info) {
        info->candidates = n;
        info->ties = ties;
    }
    return MQ_OK;
}

int topk_select(const DevState* s, const int32_t* vals, const int32_t* payload, uint64_t n, uint64_t m, int desc,
                uint64_t cap, int32_t* vals_out, int32_t* pay_out, mq_topk_info* info, hipStream_t st) {
    Scratch sc(st);
    const uint32_t flip = 0x80000000u ^ (desc ? ~0u : 0u);
    const bool vec = aligned16(vals);
    uint32_t g;
    uint64_t rpb;
    geometry(s, n, vec ? reinterpret_cast<const void*>(&k_topk_hist<true>) : reinterpret_cast<const void*>(&k_topk_hist<false>),
             &g, &rpb, (uint64_t)kTopU * kTileRows);
    uint32_t* tabs = static_cast<uint32_t*>(sc.get((size_t)g * kBins * 4));
    u64* counts = static_cast<u64*>(sc.get(kBins * 8));
    uint32_t* blk = static_cast<uint32_t*>(sc.get((size_t)g * 8));
    if (!tabs || !counts || !blk) return set_err(MQ_ENOMEM, "mq_topk: scratch allocation failed");
    uint32_t *blk_below = blk, *blk_in = blk + g;

    static thread_local u64 hc[kBins];
    uint32_t mask = 0, pfx = 0;
    uint64_t below = 0, in_bin = 0;
    int levels = 0;
    for (int L = 0; L < 3; L++) {
        const int shift = kLevels[L].shift;
        const uint32_t bins = kLevels[L].bins;
        if (vec)
            hipLaunchKernelGGL((k_topk_hist<true>), dim3(g), dim3(kTPB), 0, st, vals, n, rpb, flip, mask, pfx, shift, bins, tabs);
        else
            hipLaunchKernelGGL((k_topk_hist<false>), dim3(g), dim3(kTPB), 0, st, vals, n, rpb, flip, mask, pfx, shift, bins, tabs);
        LAUNCHCHK("k_topk_hist");
        hipLaunchKernelGGL(k_topk_fold, dim3((bins + kFoldBins - 1) / kFoldBins), dim3(kTPB), 0, st, tabs, g, bins, counts);
        LAUNCHCHK("k_topk_fold");
        HIPCHK(hipMemcpyAsync(hc, counts, (size_t)bins * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        // the bin that holds the m-th key: `need` more rows are wanted from this prefix
        const uint64_t need = m - below;
        uint64_t acc = 0;
        uint32_t B = bins;
        for (uint32_t b = 0; b < bins; b++) {
            if (acc + hc[b] >= need) {
                B = b;
                break;
            }
            acc += hc[b];
        }
        if (B == bins) return set_err(MQ_EHIP, "mq_topk: level %d counted %llu rows, %llu wanted", L, (u64)acc, (u64)need);
        below += acc;
        in_bin = hc[B];
        hipLaunchKernelGGL(k_topk_pick, dim3((g + kWaves - 1) / kWaves), dim3(kTPB), 0, st, tabs, g, bins, B, L == 0,
                           blk_below, blk_in);
        LAUNCHCHK("k_topk_pick");
        pfx |= B << shift;
        mask |= (bins - 1) << shift;
        levels = L + 1;
        if (in_bin <= cap) break;
    }
    // Rows on the boundary prefix: all of them when they fit the cap, else (three levels:
    // the prefix is one value) the first r in input order.
    const uint64_t r = m - below;  // 1 .. in_bin
    const uint64_t take = in_bin <= cap ? in_bin : r;
    const uint64_t cand = below + take;  // <= n
    hipLaunchKernelGGL(k_topk_scan, dim3(1), dim3(kTPB), 0, st, blk_below, blk_in, g);
    LAUNCHCHK("k_topk_scan");
    int32_t* c_key = static_cast<int32_t*>(sc.get(cand * 4));
    int32_t* c_pay = static_cast<int32_t*>(sc.get(cand * 4));
    if (!c_key || !c_pay) return set_err(MQ_ENOMEM, "mq_topk: candidate buffers allocation failed");
    if (vec)
        hipLaunchKernelGGL((k_topk_collect<true>), dim3(g), dim3(kTPB), 0, st, vals, payload, n, rpb, flip, mask, pfx,
                           (uint32_t)take, blk_below, blk_in, (uint32_t)cand, c_key, c_pay);
    else
        hipLaunchKernelGGL((k_topk_collect<false>), dim3(g), dim3(kTPB), 0, st, vals, payload, n, rpb, flip, mask, pfx,
                           (uint32_t)take, blk_below, blk_in, (uint32_t)cand, c_key, c_pay);
    LAUNCHCHK("k_topk_collect");
    uint64_t ties = 0;
    const bool all = in_bin <= cap;  // else no row equal to T is among the candidates past m
    const int rc = finish(sc, c_key, cand, c_pay, m, desc ? ~0u : 0u, vals_out, pay_out, info && all ? &ties : nullptr, st);
    if (rc) return rc;
    if (info) {
        info->candidates = cand;
        info->ties = all ? ties : in_bin - r;
        info->levels = levels;
    }
    return MQ_OK;
}

}  // namespace

extern "C" {

uint64_t mq_topk_default_cap(void) { return kDefaultCap; }

int mq_topk_auto_path(uint64_t n, uint64_t k, uint64_t cand_cap) {
    const uint64_t m = k < n ? k : n;
    uint64_t cap = cand_cap ? cand_cap : kDefaultCap;
    if (cap > kMaxCap) cap = kMaxCap;
    return m + cap > n / MQ_TOPK_SORT_DIV ? MQ_TOPK_SORT : MQ_TOPK_SELECT;
}

int mq_topk(const int32_t* d_vals, const int32_t* d_payload, uint64_t n, uint64_t k, int descending, int path,
            uint64_t cand_cap, int32_t* d_vals_out, int32_t* d_payload_out, mq_topk_info* h_info, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (h_info) memset(h_info, 0, sizeof *h_info);
    if (path != MQ_TOPK_AUTO && path != MQ_TOPK_SELECT && path != MQ_TOPK_SORT)
        return set_err(MQ_EINVAL, "mq_topk: path %d", path);
    if (n >= (1ull << 31)) return set_err(MQ_EINVAL, "mq_topk: n >= 2^31");
    if (n && !d_vals) return set_err(MQ_EINVAL, "mq_topk: NULL column");
    if ((reinterpret_cast<uintptr_t>(d_vals) & 3u) || (reinterpret_cast<uintptr_t>(d_payload) & 3u))
        return set_err(MQ_EINVAL, "mq_topk: column not 4-byte aligned");
    const uint64_t m = k < n ? k : n;
    uint64_t cap = cand_cap ? cand_cap : kDefaultCap;
    if (cap > kMaxCap) cap = kMaxCap;
    const int taken = path != MQ_TOPK_AUTO ? path : mq_topk_auto_path(n, k, cap);
    if (h_info) {
        h_info->m = m;
        h_info->path = taken;
    }
    if (m == 0) return MQ_OK;
    hipStream_t st = (hipStream_t)stream;
    const int desc = descending != 0;
    return taken == MQ_TOPK_SORT ? topk_sort(s, d_vals, d_payload, n, m, desc, d_vals_out, d_payload_out, h_info, st)
                                 : topk_select(s, d_vals, d_payload, n, m, desc, cap, d_vals_out, d_payload_out, h_info, st);
}

}  // extern "C"
