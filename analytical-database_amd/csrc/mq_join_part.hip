// mq_join_part.hip — the hash join's window-partitioned half: the stable
// LSD partition of build words and probe keys by table window, the kernels that build,
// check or join one window at a time in LDS, the inverse passes that take the results
// back to probe order (the last one fused with the pair write), and their host drivers.
// mq_join.hip decides when each is used (mq_join_impl.h).

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mq_common.h"
#include "mq_device.h"
#include "mq_join_impl.h"

namespace {

using namespace mqj;

// Partition tiles (TPB x kSortItems rows). Round 6, 2^28 joins alternating on one box
// (unique / many-to-many ms): build words and probe keys in 4096-row tiles 8.68 / 10.47;
// probe keys of u32-result joins in 8192-key tiles (a digit's run of keys ~128 B, a whole
// line, not 64 B) 8.29 / 10.37; build words in 8192-word tiles as well 7.85 / 10.17; the
// probe passes recording their places (k_pwin_scatter, the inverse passes without keys,
// hashing or ranking: their LDS fell from 85 to 41-74 KB) 7.62 / 10.0, and then the u64-
// result probes in 8192-key tiles too 7.59 / 9.29. Not kept: u32 probes in 16384-key
// tiles 8.84.
template <typename RT>
constexpr int probe_tpb() { return 512; }
// a deferred probe's tile width by its mode (dmode 0: u32 results), and a probe's tiles
constexpr int deferred_tpb(int dmode) { return dmode == 0 ? probe_tpb<uint32_t>() : probe_tpb<u64>(); }
uint64_t probe_tiles(uint64_t n2, int tpb) { return ceil_div(n2, (uint64_t)tpb * kSortItems); }
constexpr int kBTPB = 512;  // the build words' partition tile: kBTPB x kSortItems

// ---- window build: stable LSD radix partition of the (key, payload) words by
// window id (8 bits per pass), then one block per window builds it in LDS ----
template <bool FROM_COLS>
__device__ __forceinline__ u64 win_elem(const int* c1, const int* p1, const u64* in, uint64_t i) {
    if constexpr (FROM_COLS) return pack_pair(c1[i], p1[i]);
    else return in[i];
}

// Tiles of TPB x kSortItems rows: the build's words in tiles of kBTPB threads, the
// probe keys in tiles of probe_tpb<RT>().
template <bool FROM_COLS, int TPB = kBTPB>
__global__ __launch_bounds__(TPB) void k_win_hist(const int* __restrict__ c1,
                                                  const u64* __restrict__ in, uint64_t n, Win t,
                                                  int shift, uint32_t* __restrict__ hist,
                                                  uint32_t ntiles) {
    __shared__ uint32_t h[kRadix];
    if (threadIdx.x < kRadix) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t tile = xcd_tile(blockIdx.x, gridDim.x);
    const uint64_t base = (uint64_t)tile * (TPB * kSortItems);
    uint32_t key[kSortItems];  // loaded before any is counted, as in k_sortw_hist
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        const uint64_t i = base + (uint64_t)k * TPB + threadIdx.x;
        const uint64_t ic = i < n ? i : n - 1;
        key[k] = FROM_COLS ? (uint32_t)__builtin_nontemporal_load(c1 + ic)
                           : (uint32_t)__builtin_nontemporal_load(in + ic);
    }
#pragma unroll
    for (int k = 0; k < kSortItems; k++)
        if (base + (uint64_t)k * TPB + threadIdx.x < n) atomicAdd(&h[(win_id(key[k], t) >> shift) & 0xFF], 1u);
    __syncthreads();
    if (threadIdx.x < kRadix) hist[(uint64_t)threadIdx.x * ntiles + tile] = h[threadIdx.x];
}

// Stable scatter (k_sortw_scatter's ballot ranking), staged through LDS so that each
// digit's run leaves the block as contiguous, coalesced stores.
template <bool FROM_COLS, int TPB = kBTPB>
__global__ __launch_bounds__(TPB) void k_win_scatter(const int* __restrict__ c1,
                                                      const int* __restrict__ p1,
                                                      const u64* __restrict__ in, uint64_t n, Win t,
                                                      int shift, const u64* __restrict__ goff,
                                                      uint32_t ntiles, u64* __restrict__ out,
                                                      int* __restrict__ pmm = nullptr) {
    constexpr int kTile = TPB * kSortItems;
    __shared__ uint32_t wcnt[TPB / 64][kRadix];
    __shared__ uint32_t loff[kRadix];
    __shared__ u64 gofs[kRadix];
    __shared__ u64 stage[kTile];
    __shared__ uint32_t wsum[kRadix / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int x = tid; x < (TPB / 64) * kRadix; x += TPB) (&wcnt[0][0])[x] = 0;
    const uint32_t tile = xcd_tile(blockIdx.x, gridDim.x);
    if (tid < kRadix) gofs[tid] = goff[(uint64_t)tid * ntiles + tile];
    __syncthreads();
    const uint64_t tile0 = (uint64_t)tile * kTile;
    const uint64_t seg = tile0 + (uint64_t)wave * (64 * kSortItems);
    u64 el[kSortItems];
    uint32_t dr[kSortItems];
    // all items loaded first (indices clamped, no branch): one round trip, not one
    // per item (the ranking's ballots kept the compiler from hoisting the loads)
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        const uint64_t i = seg + (uint64_t)k * 64 + lane;
        el[k] = win_elem<FROM_COLS>(c1, p1, in, i < n ? i : n - 1);
    }
    if (FROM_COLS && pmm) {
        // the payloads' range (a value outside it marks a miss, k_win_join): per block,
        // then one atomic pair into 64 spread slots (one address for every wave made the
        // pass 5.5x slower); the host folds the slots
        int mn = INT32_MAX, mx = INT32_MIN;
#pragma unroll
        for (int k = 0; k < kSortItems; k++) {  // (clamped rows repeat row n - 1: harmless)
            const int v = (int)(el[k] >> 32);
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
        }
        __shared__ int smm[2][TPB / 64];
        if (lane == 0) smm[0][wave] = mn, smm[1][wave] = mx;
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int w = 1; w < TPB / 64; w++) {
                mn = smm[0][w] < mn ? smm[0][w] : mn;
                mx = smm[1][w] > mx ? smm[1][w] : mx;
            }
            atomicMin(pmm + (tile & 63), mn);
            atomicMax(pmm + 64 + (tile & 63), mx);
        }
    }
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        const uint64_t i = seg + (uint64_t)k * 64 + lane;
        const bool valid = i < n;
        const uint32_t d = (win_id((uint32_t)el[k], t) >> shift) & 0xFF;
        const u64 peers = match_any8(d, __ballot(valid));
        const uint32_t lt = lanes_below(peers);
        const uint32_t cur = wcnt[wave][d];
        __builtin_amdgcn_wave_barrier();
        if (valid && lt == 0) wcnt[wave][d] = cur + (uint32_t)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
        dr[k] = valid ? ((d << 16) | (cur + lt)) : 0xFFFFFFFFu;
    }
    __syncthreads();
    tile_digit_offsets<TPB>(wcnt, loff, wsum, tid);
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        if (dr[k] != 0xFFFFFFFFu) {
            const uint32_t d = dr[k] >> 16, r = dr[k] & 0xFFFF;
            stage[loff[d] + wcnt[wave][d] + r] = el[k];
        }
    }
    __syncthreads();
    const uint64_t tn = n - tile0 < (uint64_t)kTile ? n - tile0 : (uint64_t)kTile;
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        const uint32_t e = (uint32_t)(k * TPB + tid);
        if (e < tn) {
            const u64 v = stage[e];
            const uint32_t d = (win_id((uint32_t)v, t) >> shift) & 0xFF;
            out[gofs[d] + (e - loff[d])] = v;
        }
    }
}

// wstart[w] = first index of window w in the partitioned words (wstart[nw] = n):
// the words are sorted by window id, so one binary search per window boundary
// (nw + 1 threads, ~28 dependent reads whose upper levels sit in L2) instead of a
// pass over all n words (0.48 ms at 2^28).
template <typename T>
__global__ __launch_bounds__(kTPB) void k_win_bounds(const T* __restrict__ in, uint64_t n, Win t,
                                                     uint32_t nw, uint32_t* __restrict__ wstart) {
    const uint32_t x = blockIdx.x * kTPB + threadIdx.x;
    if (x > nw) return;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (win_id((uint32_t)in[mid], t) < x) lo = mid + 1;
        else hi = mid;
    }
    wstart[x] = (uint32_t)lo;
}

// One block per window: insert the window's words into an LDS table with LDS CAS,
// 1024 threads so two 64 KB-LDS blocks still fill a CU with 32 waves (measured
// 3.3 ms at 256 threads for 2^28 rows),
// then store the whole window (coalesced). Duplicates, the empty marker and an
// overfull window set *general.
__global__ __launch_bounds__(kWinTPB) void k_win_build(const u64* __restrict__ in,
                                                    const uint32_t* __restrict__ wstart,
                                                    u64* __restrict__ words, Win t,
                                                    uint32_t* __restrict__ general) {
    __shared__ u64 tab[1 << kWinLog];
    // A full bucket records in its slot order whether any key homed there went on
    // past it (then key(slot 0) > key(slot 1), else <; the keys are distinct), so a
    // probe that misses in a full bucket without overflow ends there (bucket_ovf).
    // An insert that lands outside its home bucket marks that bucket.
    __shared__ uint8_t ovf[(1 << kWinLog) / kBucket];
    const uint32_t W = (uint32_t)t.wmask + 1;
    const uint32_t w = blockIdx.x;
    for (uint32_t x = threadIdx.x; x < W; x += kWinTPB) tab[x] = kEmpty;
    for (uint32_t x = threadIdx.x; x < W / kBucket; x += kWinTPB) ovf[x] = 0;
    __syncthreads();
    const uint32_t b = wstart[w], e = wstart[w + 1];
    if (e - b > W - W / 4) {  // over 3/4 full: probes would run long (adversarial keys)
        if (threadIdx.x == 0) *general = 1;
    } else {
        // at most 3/4 of W words: every thread's (<= W / kWinTPB) words are loaded
        // before any is inserted (one round trip, not one per word)
        constexpr int kPer = (1 << kWinLog) / kWinTPB;
        u64 vs[kPer];
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            const uint32_t i = b + threadIdx.x + (uint32_t)k * kWinTPB;
            vs[k] = i < e ? in[i] : kEmpty;
        }
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            if (b + threadIdx.x + (uint32_t)k * kWinTPB >= e) break;
            const u64 v = vs[k];
            if (v == kEmpty) {
                *general = 1;
                continue;
            }
            const uint32_t key = (uint32_t)v;
            const uint32_t h0 = (uint32_t)ht_home(key, t.wmask);
            uint32_t h = h0;
            for (uint32_t step = 0; step < W; step++) {
                const u64 old = atomicCAS(&tab[h], kEmpty, v);
                if (old == kEmpty) {
                    if (step >= kBucket) ovf[h0 / kBucket] = 1;
                    break;
                }
                if ((uint32_t)old == key) {
                    *general = 1;
                    break;
                }
                h = (h + 1) & (W - 1);
            }
        }
    }
    __syncthreads();
    for (uint32_t bk = threadIdx.x; bk < W / kBucket; bk += kWinTPB) {
        const uint32_t s0 = bk * kBucket;
        const u64 a = tab[s0], c = tab[s0 + 1];
        if (a == kEmpty || c == kEmpty || tab[s0 + 2] == kEmpty || tab[s0 + 3] == kEmpty) continue;
        if (((uint32_t)a > (uint32_t)c) != (ovf[bk] != 0)) tab[s0] = c, tab[s0 + 1] = a;
    }
    __syncthreads();
    u64* dst = words + (uint64_t)w * W;
    for (uint32_t x = threadIdx.x; x < W; x += kWinTPB) dst[x] = tab[x];
}

// ---- the partitioned unique probe (round 5) ----
// A probe row's bucket read is a random 128-B line fetch from a table far beyond the
// Infinity Cache: 2^28 probes moved ~34 GB for 8 GB of buckets (PMC). Instead the probe
// keys take the build's window partition (the same LSD passes, u32 keys), one block per
// window builds the window's table in LDS from the build's partitioned words and probes
// it with the window's probe keys (k_win_join: no global table is ever written or
// read), and the results go back to probe order by running the passes backwards
// (k_pwin_gather). Everything moves as streams.

// One pass of the probe keys by window-id digit (round 6 form). The pass records each
// row's place in its tile's digit order (perm, u16) for the inverse passes, which then
// neither hash nor rank: they read 2 B a row instead of the 4-B keys. STABLE: rows of a
// digit keep their order (ballot match-any ranks), which every pass after the first
// needs, so that the windows come out whole (LSD); the first pass's keys need no order
// within a digit (each key's result is its own), so there a key takes its place by one
// LDS atomic.
template <int TPB, bool STABLE>
__global__ __launch_bounds__(TPB) void k_pwin_scatter(const uint32_t* __restrict__ in, uint64_t n, Win t, int shift,
                                                      const u64* __restrict__ goff, uint32_t ntiles,
                                                      uint32_t* __restrict__ out, uint16_t* __restrict__ perm) {
    constexpr int kTile = TPB * kSortItems, kW = STABLE ? TPB / 64 : 1;
    static_assert(kTile <= 65536, "u16 places");
    __shared__ uint32_t wcnt[kW][kRadix];  // per wave (STABLE) or per tile
    __shared__ uint32_t loff[kRadix];
    __shared__ u64 gofs[kRadix];
    __shared__ uint32_t stage[kTile];
    __shared__ uint8_t sdig[kTile];
    __shared__ uint32_t wsum[kRadix / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t tile = xcd_tile(blockIdx.x, gridDim.x);
    for (int x = tid; x < kW * kRadix; x += TPB) (&wcnt[0][0])[x] = 0;
    if (tid < kRadix) gofs[tid] = goff[(uint64_t)tid * ntiles + tile];
    __syncthreads();
    const uint64_t tile0 = (uint64_t)tile * kTile;
    // rows: STABLE, wave w owns 64 * kSortItems consecutive rows (ranks in row order);
    // else thread-strided
    auto row = [&](int k) -> uint64_t {
        return STABLE ? tile0 + (uint64_t)wave * (64 * kSortItems) + (uint64_t)k * 64 + lane
                      : tile0 + (uint64_t)k * TPB + tid;
    };
    uint32_t el[kSortItems], dr[kSortItems];
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        const uint64_t i = row(k);
        el[k] = __builtin_nontemporal_load(in + (i < n ? i : n - 1));
    }
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        const uint64_t i = row(k);
        const bool valid = i < n;
        const uint32_t d = (win_id(el[k], t) >> shift) & 0xFF;
        if constexpr (STABLE) {
            const u64 peers = match_any8(d, __ballot(valid));
            const uint32_t lt = lanes_below(peers);
            const uint32_t cur = wcnt[wave][d];
            __builtin_amdgcn_wave_barrier();
            if (valid && lt == 0) wcnt[wave][d] = cur + (uint32_t)__popcll(peers);
            __builtin_amdgcn_wave_barrier();
            dr[k] = valid ? ((d << 16) | (cur + lt)) : 0xFFFFFFFFu;
        } else {
            dr[k] = valid ? (d << 16) | atomicAdd(&wcnt[0][d], 1u) : 0xFFFFFFFFu;
        }
    }
    __syncthreads();
    if constexpr (STABLE) tile_digit_offsets<TPB>(wcnt, loff, wsum, tid);
    else digit_scan(wcnt[0], loff, wsum, tid);
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        const uint64_t i = row(k);
        if (dr[k] != 0xFFFFFFFFu) {
            const uint32_t d = dr[k] >> 16;
            const uint32_t sp = loff[d] + (STABLE ? wcnt[wave][d] : 0u) + (dr[k] & 0xFFFF);
            stage[sp] = el[k];
            sdig[sp] = (uint8_t)d;
            perm[i] = (uint16_t)sp;
        }
    }
    __syncthreads();
    const uint64_t tn = n - tile0 < (uint64_t)kTile ? n - tile0 : (uint64_t)kTile;
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        const uint32_t e = (uint32_t)(k * TPB + tid);
        if (e < tn) {
            const uint32_t d = sdig[e];
            out[gofs[d] + (e - loff[d])] = stage[e];
        }
    }
}

// The inverse passes' view of a tile: gofs[d] = where digit d's run of the tile starts in
// the pass's output, loff[d] its tile-local start (from the pass's scanned offsets: a
// run's length is the next offset's distance), sdig[e] = the digit of place e.
__device__ __forceinline__ void tile_runs(const u64* __restrict__ goff, uint32_t ntiles, uint32_t tile, uint64_t n,
                                          u64* gofs, uint32_t* cnt, uint32_t* loff, uint8_t* sdig, uint32_t* wsum,
                                          int tid) {
    if (tid < kRadix) {
        const uint64_t x = (uint64_t)tid * ntiles + tile;
        const u64 g = goff[x], gn = x + 1 < (uint64_t)kRadix * ntiles ? goff[x + 1] : n;
        gofs[tid] = g;
        cnt[tid] = (uint32_t)(gn - g);
    }
    __syncthreads();
    digit_scan(cnt, loff, wsum, tid);
    if (tid < kRadix)
        for (uint32_t e = loff[tid], e1 = loff[tid] + cnt[tid]; e < e1; e++) sdig[e] = (uint8_t)tid;
    __syncthreads();
}

// Persistent window kernels (round 5): a window is a small job (8192 slots' worth of
// build words, ~4096 on average, and ~4096 probe keys), so a block walks windows w,
// w + G, ... (G = two blocks a CU). kWinPer build words and kJoinPer probe keys a thread
// cover 8192 / 5120 per window; probe keys past that are loaded in place. Round 5 issued
// the next window's loads into registers before the current window's LDS work; that
// took the kernels to 88-90 VGPRs, so only one 1024-lane block fitted a CU (the grid's
// second half waited for the first). Round 6 drops the register prefetch and caps the
// kernels at 8 waves a SIMD (64 VGPRs, no spills): two blocks share a CU and cover each
// other's loads. 2^28, alternating on one box: unique 7.59 -> 7.43 ms, many-to-many
// 9.18 -> 8.74 ms; the prefetch kept under the same cap spilled (40-52 B a lane) and
// measured 7.72 / 9.86.
//
// In LDS a window is not an open-addressing table but its words grouped by bucket (a
// counting sort, CSR): kCsrBuckets buckets by hash, one LDS atomic add per word gives
// its rank, a scan the buckets' starts, a store its place. A lookup reads its bucket's
// bounds and then the bucket's words (about one), which are independent reads. The
// table's CAS insert and linear probe were chains of dependent LDS round trips: the
// first form of these kernels (one window per block, k_win_build's CAS insert) took
// 1.6 ms for the check and 3.3 ms for the join at 2^28 rows.
constexpr int kJoinPer = 5;
constexpr int kWinPer = (1 << kWinLog) / kWinTPB;
constexpr uint32_t kCsrBuckets = 1u << (kWinLog - 1);        // 4096: about one word a bucket
constexpr uint32_t kCsrCap = (1u << kWinLog) - (1u << kWinLog) / 4;  // 6144 words: the 3/4 rule

__device__ __forceinline__ uint32_t csr_bucket(uint32_t key, const Win& t) {
    return (uint32_t)((hash32(key) & t.wmask) >> 1);
}

__device__ __forceinline__ void win_load(const u64* __restrict__ in, uint32_t b, uint32_t e, u64 (&v)[kWinPer]) {
#pragma unroll
    for (int k = 0; k < kWinPer; k++) {
        const uint32_t i = b + threadIdx.x + (uint32_t)k * kWinTPB;
        v[k] = i < e ? __builtin_nontemporal_load(in + i) : kEmpty;
    }
}

// The window's c words (c <= kCsrCap, threads' words vs[k] = word threadIdx + k * kWinTPB)
// grouped by bucket into csr; boff[b] .. boff[b + 1] = bucket b's words. Ends synced.
// cidx (when not null): each grouped word's index in the window's stretch (input order).
__device__ __forceinline__ void csr_build(const u64 (&vs)[kWinPer], uint32_t c, const Win& t, u64* csr,
                                          uint32_t* boff, uint32_t* wsum, uint16_t* cidx = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t x = tid; x <= kCsrBuckets; x += kWinTPB) boff[x] = 0;
    __syncthreads();
    uint32_t rk[kWinPer];
#pragma unroll
    for (int k = 0; k < kWinPer; k++) {
        const uint32_t i = (uint32_t)tid + (uint32_t)k * kWinTPB;
        rk[k] = i < c ? atomicAdd(&boff[csr_bucket((uint32_t)vs[k], t)], 1u) : 0u;
    }
    __syncthreads();
    // exclusive scan of the kCsrBuckets counts: 4 consecutive a thread
    constexpr int kQ = (int)(kCsrBuckets / kWinTPB);
    uint32_t cnt[kQ], tot = 0;
#pragma unroll
    for (int q = 0; q < kQ; q++) {
        cnt[q] = boff[tid * kQ + q];
        tot += cnt[q];
    }
    uint32_t incl = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(incl, off, 64);
        if (lane >= off) incl += y;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t run = incl - tot;
    for (int w = 0; w < wave; w++) run += wsum[w];
#pragma unroll
    for (int q = 0; q < kQ; q++) {
        boff[tid * kQ + q] = run;
        run += cnt[q];
    }
    if (tid == kWinTPB - 1) boff[kCsrBuckets] = run;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kWinPer; k++) {
        const uint32_t i = (uint32_t)tid + (uint32_t)k * kWinTPB;
        if (i < c) {
            const uint32_t x = boff[csr_bucket((uint32_t)vs[k], t)] + rk[k];
            csr[x] = vs[k];
            if (cidx) cidx[x] = (uint16_t)i;
        }
    }
    __syncthreads();
}

// One window at a time per block: the window's build words grouped in LDS, then each of
// the window's probe keys (partitioned order) looks itself up in its bucket. r[i] =
// payload << 32 | 1 on a hit, 0 on a miss. The build was not checked: a probe key that
// finds two build words sets bit 0 of *flag (the caller probes again with the duplicate-
// capable k_win_join_runs), a window over kCsrCap words bit 1 (the caller rebuilds
// without the partition; the table's empty word is an ordinary word here).
template <typename RT>
__global__ __launch_bounds__(kWinTPB) __attribute__((amdgpu_waves_per_eu(8))) void k_win_join(const u64* __restrict__ bwords,
                                                      const uint32_t* __restrict__ bstart,
                                                      const uint32_t* __restrict__ pkeys,
                                                      const uint32_t* __restrict__ pstartw, uint32_t nwin, Win t,
                                                      RT* __restrict__ r, uint32_t* __restrict__ flag,
                                                      uint32_t sentinel, unsigned long long* __restrict__ mtot) {
    __shared__ u64 csr[kCsrCap];
    __shared__ uint32_t boff[kCsrBuckets + 1];
    __shared__ uint32_t wsum[kWinTPB / 64];
    const uint32_t G = gridDim.x;
    uint32_t w = blockIdx.x;
    if (w >= nwin) return;
    auto key_load = [&](uint32_t pb, uint32_t pe, uint32_t (&key)[kJoinPer]) {
#pragma unroll
        for (int k = 0; k < kJoinPer; k++) {
            const uint32_t i = pb + threadIdx.x + (uint32_t)k * kWinTPB;
            key[k] = i < pe ? __builtin_nontemporal_load(pkeys + i) : 0u;
        }
    };
    bool dup = false, overfull = false;
    unsigned long long nhit = 0;  // the window joins' pairs (M, for the fused write)
    // a key on two build words shows up only where a probe key matches it (duplicates no
    // probe row meets do not change the unique output): then the flag
    auto lookup = [&](uint32_t key) -> RT {
        const uint32_t bk = csr_bucket(key, t);
        const uint32_t x0 = boff[bk], x1 = boff[bk + 1];
        u64 out = 0;
        uint32_t hits = 0;
        for (uint32_t x = x0; x < x1; x++) {
            const u64 v = csr[x];
            if ((uint32_t)v == key) out = (v & 0xFFFFFFFF00000000ull) | 1ull, hits++;
        }
        dup |= hits > 1;
        nhit += hits ? 1u : 0u;
        if constexpr (sizeof(RT) == 4) return hits ? (uint32_t)(out >> 32) : sentinel;
        else return out;
    };
    // The loads' order decides what the wait-count pass can overlap (it waits for a
    // register's load with vmcnt(n), n = the younger memory operations, unknown past a
    // data-dependent number of stores): the next window's build words are issued at the
    // top and waited for after this window's grouping, the next window's probe keys
    // after this window's stores; nothing waits on this window's stores.
    for (; w < nwin; w += G) {
        const uint32_t b = bstart[w], e = bstart[w + 1], pb = pstartw[w], pe = pstartw[w + 1];
        u64 vs[kWinPer];
        uint32_t key[kJoinPer];
        win_load(bwords, b, e, vs);
        key_load(pb, pe, key);
        const bool over = e - b > kCsrCap;  // uniform: an overfull window (its results are dropped)
        if (!over) csr_build(vs, e - b, t, csr, boff, wsum);
        if (over) {
            overfull = true;
        } else {
#pragma unroll
            for (int k = 0; k < kJoinPer; k++) {
                const uint32_t i = pb + threadIdx.x + (uint32_t)k * kWinTPB;
                if (i < pe) __builtin_nontemporal_store(lookup(key[k]), r + i);
            }
            for (uint32_t i = pb + threadIdx.x + (uint32_t)kJoinPer * kWinTPB; i < pe; i += kWinTPB)
                __builtin_nontemporal_store(lookup(__builtin_nontemporal_load(pkeys + i)), r + i);
            __syncthreads();
        }
    }
    if (dup || overfull) atomicOr(flag, (dup ? 1u : 0u) | (overfull ? 2u : 0u));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nhit += __shfl_xor(nhit, o, 64);
    if ((threadIdx.x & 63) == 0 && nhit) atomicAdd(mtot, nhit);
}

// The partitioned probe of a windowed RUNS table (duplicate keys, k_win_build_runs: the
// window's slots hold {key, start << 4 | length}): the window's 64 KB slice of the
// global table is loaded into LDS whole (coalesced) and each of the window's probe keys
// follows the table's own probe sequence there (home bucket, linear inside the window,
// an empty slot ends it). r[i] = the slot's packed run, 0 = no match (a run is never
// empty, so a hit's payload is never 0). (Round 5's u64 form carried short runs' build
// positions from the run array; round 6's k_win_join_runs does that without the table.)
template <typename RT>
__global__ __launch_bounds__(kWinTPB) void k_win_probe_tab(const u64* __restrict__ words,
                                                           const uint32_t* __restrict__ pkeys,
                                                           const uint32_t* __restrict__ pstartw, uint32_t nwin, Win t,
                                                           RT* __restrict__ r) {
    static_assert(sizeof(RT) == 4, "packed runs");
    __shared__ u64 tab[1 << kWinLog];
    const uint32_t W = (uint32_t)t.wmask + 1, G = gridDim.x;
    uint32_t w = blockIdx.x;
    if (w >= nwin) return;
    auto key_load = [&](uint32_t pb, uint32_t pe, uint32_t (&key)[kJoinPer]) {
#pragma unroll
        for (int k = 0; k < kJoinPer; k++) {
            const uint32_t i = pb + threadIdx.x + (uint32_t)k * kWinTPB;
            key[k] = i < pe ? __builtin_nontemporal_load(pkeys + i) : 0u;
        }
    };
    auto lookup = [&](uint32_t key) -> RT {
        uint32_t h = (uint32_t)ht_home(key, t.wmask);
        uint32_t pk = 0;
        for (uint32_t step = 0; step < W; step++) {
            const u64 v = tab[h];
            if (v == kEmpty) break;
            if ((uint32_t)v == key) {
                pk = (uint32_t)(v >> 32);
                break;
            }
            h = (h + 1) & (W - 1);
        }
        return pk;
    };
    uint32_t pb = pstartw[w], pe = pstartw[w + 1];
    u64 vs[kWinPer];
    uint32_t key[kJoinPer];
    win_load(words + (uint64_t)w * W, 0, W, vs);
    key_load(pb, pe, key);
    uint32_t pbn = 0, pen = 0;
    if (w + G < nwin) pbn = pstartw[w + G], pen = pstartw[w + G + 1];
    __builtin_amdgcn_s_waitcnt(0);  // (see k_win_join)
    for (; w < nwin; w += G) {
        u64 vn[kWinPer];
        win_load(words + (uint64_t)(w + G < nwin ? w + G : w) * W, 0, w + G < nwin ? W : 0, vn);
        uint32_t pbnn = 0, penn = 0;
        if (w + 2 * G < nwin) pbnn = pstartw[w + 2 * G], penn = pstartw[w + 2 * G + 1];
#pragma unroll
        for (int k = 0; k < kWinPer; k++) tab[threadIdx.x + (uint32_t)k * kWinTPB] = vs[k];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kWinPer; k++) {
            asm volatile("" : "+v"(vn[k]));  // the next slice waited for here, not behind the stores
            vs[k] = vn[k];
        }
#pragma unroll
        for (int k = 0; k < kJoinPer; k++) {
            const uint32_t i = pb + threadIdx.x + (uint32_t)k * kWinTPB;
            if (i < pe) __builtin_nontemporal_store(lookup(key[k]), r + i);
        }
        for (uint32_t i = pb + threadIdx.x + (uint32_t)kJoinPer * kWinTPB; i < pe; i += kWinTPB)
            __builtin_nontemporal_store(lookup(__builtin_nontemporal_load(pkeys + i)), r + i);
        __syncthreads();
        key_load(pbn, pen, key);
        pb = pbn, pe = pen, pbn = pbnn, pen = penn;
    }
}

// The partitioned probe for DUPLICATE build keys (round 6): no runs table. The build
// words stay partitioned by window as for unique keys (the stable LSD passes keep a
// window's words in input order, their stretch index i); per window the block groups
// them by bucket in LDS (csr_build, with each word's i) and answers each probe key of
// the window from its bucket: the words of equal key are the key's build rows, ordered
// by i (build-insertion order, query.c:669-681). r[k] is the run2 record the gathers
// and the write read: {p0, S} for one row, {p0, p1} for two (in order), {S, (b + s) << 4
// | L} for L = 3..14 rows, whose build positions are in bpos[b + s ...] in insertion
// order (s = the run's place when the bucket is ordered by (key, i), so every run has its
// own stretch inside the window's; written by the probe keys that meet the run, each the
// same values), and {S, 0} for a miss. S: a value outside the build payloads (the host
// checks one exists). A window over kCsrCap words or a probed key on 15+ rows sets *flag
// (the caller rebuilds on the sorted runs); *mtot += the pairs (sum of L over the probe
// keys).
// Replaces k_win_build_runs (the 4 GB runs table written by the build, 1.9 ms at 2^28)
// and k_win_probe_tab (reading it back, 1.76 ms).
__global__ __launch_bounds__(kWinTPB) __attribute__((amdgpu_waves_per_eu(8))) void k_win_join_runs(const u64* __restrict__ bwords,
                                                           const uint32_t* __restrict__ bstart,
                                                           const uint32_t* __restrict__ pkeys,
                                                           const uint32_t* __restrict__ pstartw, uint32_t nwin, Win t,
                                                           u64* __restrict__ r, int* __restrict__ bpos,
                                                           uint32_t* __restrict__ flag, unsigned long long* mtot,
                                                           uint32_t S) {
    __shared__ u64 csr[kCsrCap];
    __shared__ uint32_t boff[kCsrBuckets + 1];
    __shared__ uint16_t cidx[kCsrCap];
    __shared__ uint32_t wsum[kWinTPB / 64];
    const uint32_t G = gridDim.x;
    uint32_t w = blockIdx.x;
    if (w >= nwin) return;
    auto key_load = [&](uint32_t pb, uint32_t pe, uint32_t (&key)[kJoinPer]) {
#pragma unroll
        for (int k = 0; k < kJoinPer; k++) {
            const uint32_t i = pb + threadIdx.x + (uint32_t)k * kWinTPB;
            key[k] = i < pe ? __builtin_nontemporal_load(pkeys + i) : 0u;
        }
    };
    bool bad = false;
    unsigned long long pairs = 0;
    // key k's words in bucket [x0, x1): count L, those below k (its run's place in the
    // bucket ordered by (key, i)), and the first two by i
    auto scan_bucket = [&](uint32_t key, uint32_t b, uint32_t x0, uint32_t x1, uint32_t& L, uint32_t& lt,
                           uint32_t& p0, uint32_t& p1) {
        // the first two matches in bucket order, then put in input order (selects, no
        // array: an insertion by index compiled to a scratch array)
        uint32_t n = 0, ia = 0, ib = 0, pa = S, pb = S;
        for (uint32_t x = x0; x < x1; x++) {
            const u64 v = csr[x];
            if ((uint32_t)v == key) {
                const uint32_t i = cidx[x], p = (uint32_t)(v >> 32);
                ia = n == 0 ? i : ia;
                pa = n == 0 ? p : pa;
                ib = n == 1 ? i : ib;
                pb = n == 1 ? p : pb;
                n++;
            }
        }
        const bool sw = n == 2 && ib < ia;
        p0 = sw ? pb : pa;
        p1 = sw ? pa : pb;
        L = n;
        lt = 0;
        if (n >= 3u) {
            // a long run: its place in the bucket ordered by (key, i), and its rows' payloads
            // written there in insertion order by every probe key that meets it (the same
            // values to the same places: no race); no key of the window pays otherwise
            for (uint32_t x = x0; x < x1; x++) lt += (uint32_t)csr[x] < key ? 1u : 0u;
            if (n < 15u)
                for (uint32_t x = x0; x < x1; x++) {
                    const u64 v = csr[x];
                    if ((uint32_t)v != key) continue;
                    const uint32_t me = cidx[x];
                    uint32_t rk = 0;
                    for (uint32_t y = x0; y < x1; y++)
                        rk += ((uint32_t)csr[y] == key && cidx[y] < me) ? 1u : 0u;
                    bpos[b + x0 + lt + rk] = (int)(uint32_t)(v >> 32);
                }
            else
                bad = true;  // not packable: the caller takes the sorted runs
        }
    };
    auto lookup = [&](uint32_t key, uint32_t b) -> u64 {
        const uint32_t bk = csr_bucket(key, t);
        const uint32_t x0 = boff[bk], x1 = boff[bk + 1];
        uint32_t L, lt, p0, p1;
        scan_bucket(key, b, x0, x1, L, lt, p0, p1);
        pairs += L;
        if (L == 0) return (u64)S;
        if (L <= 2) return (u64)p0 | ((u64)p1 << 32);
        return (u64)S | ((u64)(((b + x0 + lt) << 4) | (L < 15u ? L : 15u)) << 32);
    };
    for (; w < nwin; w += G) {  // (no register prefetch of the next window: see k_win_join)
        const uint32_t b = bstart[w], e = bstart[w + 1], pb = pstartw[w], pe = pstartw[w + 1];
        u64 vs[kWinPer];
        uint32_t key[kJoinPer];
        win_load(bwords, b, e, vs);
        key_load(pb, pe, key);
        const uint32_t c = e - b;
        const bool over = c > kCsrCap;  // uniform
        if (!over) csr_build(vs, c, t, csr, boff, wsum, cidx);
        if (over) {
            bad = true;
        } else {
#pragma unroll
            for (int k = 0; k < kJoinPer; k++) {
                const uint32_t i = pb + threadIdx.x + (uint32_t)k * kWinTPB;
                if (i < pe) __builtin_nontemporal_store(lookup(key[k], b), r + i);
            }
            for (uint32_t i = pb + threadIdx.x + (uint32_t)kJoinPer * kWinTPB; i < pe; i += kWinTPB)
                __builtin_nontemporal_store(lookup(__builtin_nontemporal_load(pkeys + i), b), r + i);
            __syncthreads();
        }
    }
    if (bad) *flag = 1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pairs += __shfl_xor(pairs, o, 64);
    if ((threadIdx.x & 63) == 0 && pairs) atomicAdd(mtot, pairs);
}

// The inverse of one k_pwin_scatter pass: perm = that pass's places (a row's place in
// its tile's digit order), rin = per-row results in the pass's output order; rout[i] =
// the result of input row i. Each digit's run of the tile is read from rin as a
// contiguous stretch (staged in LDS by place) and every row takes its own value back.
// FINAL (the pass over the probe column itself): per row the payload (pstart) and, per
// 64 rows, the hit word.
// RUNS (with FINAL): rin holds packed runs (0 = no match); per row pstart = the packed
// run and per 64 rows wcnt = the sum of their run lengths, as k_ht_probe_unique<true>
// leaves them for the packed-runs write (hits is then that wcnt, as u32).
template <bool FINAL, typename RT, bool RUNS, int TPB>
__global__ __launch_bounds__(TPB) void k_pwin_gather(const uint16_t* __restrict__ perm, uint64_t n,
                                                     const u64* __restrict__ goff, uint32_t ntiles,
                                                     const RT* __restrict__ rin, RT* __restrict__ rout,
                                                     uint32_t* __restrict__ pstart, u64* __restrict__ hits,
                                                     uint32_t sentinel) {
    constexpr int kTile = TPB * kSortItems;
    __shared__ uint32_t cnt[kRadix];
    __shared__ uint32_t loff[kRadix];
    __shared__ u64 gofs[kRadix];
    __shared__ RT stage[kTile];
    __shared__ uint8_t sdig[kTile];
    __shared__ uint32_t wsum[kRadix / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t tile = xcd_tile(blockIdx.x, gridDim.x);
    const uint64_t tile0 = (uint64_t)tile * kTile;
    const uint64_t seg = tile0 + (uint64_t)wave * (64 * kSortItems);
    uint32_t sp[kSortItems];  // each row's place in the tile's digit order
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        const uint64_t i = seg + (uint64_t)k * 64 + lane;
        sp[k] = __builtin_nontemporal_load(perm + (i < n ? i : n - 1));
    }
    tile_runs(goff, ntiles, tile, n, gofs, cnt, loff, sdig, wsum, tid);
    const uint64_t tn = n - tile0 < (uint64_t)kTile ? n - tile0 : (uint64_t)kTile;
    {
        RT v[kSortItems];  // all reads in flight first
#pragma unroll
        for (int k = 0; k < kSortItems; k++) {
            const uint32_t e = (uint32_t)(k * TPB + tid);
            const uint32_t d = e < tn ? sdig[e] : 0u;
            v[k] = e < tn ? __builtin_nontemporal_load(rin + gofs[d] + (e - loff[d])) : (RT)0;
        }
#pragma unroll
        for (int k = 0; k < kSortItems; k++) stage[k * TPB + tid] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        const uint64_t i = seg + (uint64_t)k * 64 + lane;
        const bool in = i < n;
        const RT v = in ? stage[sp[k]] : (RT)0;
        if constexpr (FINAL && RUNS && sizeof(RT) == 8) {
            // run2 records: pstart = a packed run (long) or just its length (one or two rows,
            // whose positions go to rout = p01), as k_join_write_runs16 reads them
            const uint32_t lo = (uint32_t)v, hi = (uint32_t)((u64)v >> 32);
            const bool direct = lo != sentinel;
            const uint32_t pk = !in ? 0u : direct ? (hi == sentinel ? 1u : 2u) : hi;
            uint32_t L = pk & 15u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) L += __shfl_xor(L, o, 64);
            if (i < n) {
                __builtin_nontemporal_store(pk, pstart + i);
                __builtin_nontemporal_store((in && direct) ? (u64)v : 0ull, reinterpret_cast<u64*>(rout) + i);
            }
            if (lane == 0 && i < n) reinterpret_cast<uint32_t*>(hits)[i >> 6] = L;
        } else if constexpr (FINAL && RUNS) {
            const uint32_t pay = (uint32_t)v;
            uint32_t L = pay & 15u;  // (a windowed runs table: every run shorter than 15)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) L += __shfl_xor(L, o, 64);
            if (i < n) __builtin_nontemporal_store(pay, pstart + i);
            if (lane == 0 && i < n) reinterpret_cast<uint32_t*>(hits)[i >> 6] = L;
        } else if constexpr (FINAL) {
            bool hit;
            uint32_t pay;
            if constexpr (sizeof(RT) == 4) {
                hit = in && (uint32_t)v != sentinel;
                pay = (uint32_t)v;
            } else {
                hit = ((u64)v & 1ull) != 0;
                pay = (uint32_t)((u64)v >> 32);
            }
            const u64 m = __ballot(hit);
            if (i < n) __builtin_nontemporal_store(pay, pstart + i);
            if (lane == 0 && i < n) hits[i >> 6] = m;
        } else {
            if (i < n) __builtin_nontemporal_store(v, rout + i);
        }
    }
}

// The last inverse pass fused with the pair write (round 6): k_pwin_gather<true>'s tile
// (its probe rows in row order; each row's result taken back from the window join's
// order) counts its pairs, learns the pairs of every earlier tile by decoupled look-back
// and writes its rows' pairs straight to out1 / out2, so neither the per-row results
// (pstart, p01: 4-12 B a row written and read back) nor the hit words, their scan and a
// separate write pass exist. MODE 0: unique, u32 results (sentinel = miss); 1: unique,
// u64 {payload << 32 | 1} (0 = miss); 2: run2 records (k_win_join_runs), runs of 3-14
// rows read from bpos. status[t] = kLbAgg | the tile's pairs, then kLbPre | the pairs of
// tiles 0..t.
// Tile order (kGwGroup): a digit's runs of neighbouring tiles share cache lines of rin,
// so neighbours should run on one XCD. Blocks are dispatched in blockIdx order, dealt
// round-robin over the 8 XCDs; in each group of 8 * kGwGroup blocks, the kGwGroup blocks
// of one XCD take kGwGroup consecutive tiles (a partial last group keeps blockIdx order).
// A tile waits only on lower tiles, whose blocks come earlier in dispatch order or in the
// same group (as k_select_stage relies on lower blocks being dispatched first). Round 6,
// 2^28 joins alternating on one box: tiles by an atomic ticket (order of block start, any
// XCD) 8.78 / 10.58 ms, groups of 4 8.70 / 10.47 (reads 1.75x -> 1.59x the design bytes,
// unique), groups of 8 8.77 / 10.62; 4 tiles a ticket in one block serialised the chain.
constexpr u64 kLbAgg = 1ull << 62, kLbPre = 2ull << 62, kLbVal = (1ull << 62) - 1;
constexpr uint32_t kGwGroup = 4;

__device__ __forceinline__ u64 lb_load(const u64* p) {
    return __hip_atomic_load(const_cast<u64*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lb_store(u64* p, u64 v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename RT, int MODE, int TPB>
__global__ __launch_bounds__(TPB) void k_pwin_gather_write(const uint16_t* __restrict__ perm, uint64_t n,
                                                            const u64* __restrict__ goff, uint32_t ntiles,
                                                            const RT* __restrict__ rin, const int* __restrict__ p2,
                                                            const int* __restrict__ bpos, uint32_t sentinel,
                                                            int* __restrict__ out1, int* __restrict__ out2,
                                                            u64* status, uint32_t* err) {
    constexpr int kTile = TPB * kSortItems;
    __shared__ uint32_t cnt[kRadix];
    __shared__ uint32_t loff[kRadix];
    __shared__ u64 gofs[kRadix];
    __shared__ RT stage[kTile];
    __shared__ uint8_t sdig[kTile];
    __shared__ uint32_t wsum[TPB / 64];
    __shared__ u64 s_excl;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t tile = blockIdx.x;  // (see kGwGroup)
    {
        constexpr uint32_t kSpan = 8u * kGwGroup;
        const uint32_t g0 = tile - tile % kSpan;
        if (g0 + kSpan <= ntiles) tile = g0 + (tile & 7u) * kGwGroup + (tile % kSpan) / 8u;
    }
    const uint64_t tile0 = (uint64_t)tile * kTile;
    const uint64_t seg = tile0 + (uint64_t)wave * (64 * kSortItems);
    uint32_t sp[kSortItems];  // each row's place in the tile's digit order
    int pv[kSortItems];       // the rows' probe positions, loaded with the places (a load at
                              // each store serialised 16 round trips a wave)
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        const uint64_t i = seg + (uint64_t)k * 64 + lane;
        sp[k] = __builtin_nontemporal_load(perm + (i < n ? i : n - 1));
        pv[k] = out2 ? __builtin_nontemporal_load(p2 + (i < n ? i : n - 1)) : 0;
    }
    tile_runs(goff, ntiles, tile, n, gofs, cnt, loff, sdig, wsum, tid);
    const uint64_t tn = n - tile0 < (uint64_t)kTile ? n - tile0 : (uint64_t)kTile;
    {
        RT v[kSortItems];
#pragma unroll
        for (int k = 0; k < kSortItems; k++) {
            const uint32_t e = (uint32_t)(k * TPB + tid);
            const uint32_t d = e < tn ? sdig[e] : 0u;
            v[k] = e < tn ? __builtin_nontemporal_load(rin + gofs[d] + (e - loff[d])) : (RT)0;
        }
#pragma unroll
        for (int k = 0; k < kSortItems; k++) stage[k * TPB + tid] = v[k];
    }
    __syncthreads();
    // each row's pair count (from its result, read from stage twice: once for the wave's
    // total, once for the write, instead of holding results, counts and prefixes in
    // registers: 229 VGPRs, 2 waves a SIMD). Counts are below 16, so a wave's prefix and
    // total are 4 bit-ballots (1 for unique keys). Row order: wave, item, lane.
    auto count_of = [&](RT v) -> uint32_t {
        if constexpr (MODE == 0) {
            return (uint32_t)v != sentinel ? 1u : 0u;
        } else if constexpr (MODE == 1) {
            return (uint32_t)((u64)v & 1ull);
        } else {
            const uint32_t lo = (uint32_t)v, hi = (uint32_t)((u64)v >> 32);
            return lo != sentinel ? (hi == sentinel ? 1u : 2u) : (hi & 15u);
        }
    };
    constexpr int kBits = MODE == 2 ? 4 : 1;
    auto wave_prefix = [&](uint32_t c, uint32_t& tot) -> uint32_t {
        uint32_t pre = 0;
        tot = 0;
#pragma unroll
        for (int b = 0; b < kBits; b++) {
            const u64 m = __ballot((c >> b) & 1u);
            pre += lanes_below(m) << b;
            tot += (uint32_t)__popcll(m) << b;
        }
        return pre;
    };
    uint32_t wrun = 0;
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        const uint64_t i = seg + (uint64_t)k * 64 + lane;
        const uint32_t c = i < n ? count_of(stage[sp[k]]) : 0u;
        uint32_t tot;
        (void)wave_prefix(c, tot);
        wrun += tot;
    }
    __syncthreads();  // (wsum reused)
    if (lane == 0) wsum[wave] = wrun;
    __syncthreads();
    uint32_t wbase = 0, ttot = 0;
#pragma unroll
    for (int w = 0; w < TPB / 64; w++) {
        wbase += w < wave ? wsum[w] : 0u;
        ttot += wsum[w];
    }
    // decoupled look-back over the earlier tiles (wave 0)
    if (wave == 0) {
        if (lane == 0) lb_store(&status[tile], (tile ? kLbAgg : kLbPre) | (u64)ttot);
        u64 acc = 0;
        int64_t j = (int64_t)tile - 1;
        uint32_t spins = 0;
        while (j >= 0) {
            const int64_t idx = j - lane;
            u64 x = idx >= 0 ? lb_load(&status[idx]) : kLbPre;
            // every lane's status published (bounded: never expected to run long)
            while (__ballot((x & ~kLbVal) == 0)) {
                if (++spins > (1u << 24)) {
                    if (lane == 0) atomicOr(err, 1u);
                    x = kLbPre;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
                if ((x & ~kLbVal) == 0) x = lb_load(&status[idx]);
            }
            const u64 pm = __ballot((x & kLbPre) != 0);
            const int stop = pm ? __ffsll((long long)pm) - 1 : 64;  // the nearest inclusive prefix
            u64 val = lane <= stop ? (x & kLbVal) : 0ull;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) val += __shfl_xor(val, o, 64);
            acc += val;
            if (pm) break;
            j -= 64;
        }
        if (lane == 0) {
            if (tile) lb_store(&status[tile], kLbPre | (acc + ttot));
            s_excl = acc;
        }
    }
    __syncthreads();
    u64 o = s_excl + wbase;  // (wave-uniform) the first pair of this wave's next item
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        const uint64_t i = seg + (uint64_t)k * 64 + lane;
        const RT v = i < n ? stage[sp[k]] : (RT)0;
        const uint32_t c = i < n ? count_of(v) : 0u;
        uint32_t tot;
        const uint32_t pre = wave_prefix(c, tot);
        if (c) {
            const u64 q = o + pre;
            const int pp = pv[k];
            if constexpr (MODE == 0) {
                out1[q] = (int)(uint32_t)v;
                if (out2) out2[q] = pp;
            } else if constexpr (MODE == 1) {
                out1[q] = (int)(uint32_t)((u64)v >> 32);
                if (out2) out2[q] = pp;
            } else {
                const uint32_t lo = (uint32_t)v, hi = (uint32_t)((u64)v >> 32);
                if (lo != sentinel) {
                    out1[q] = (int)lo;
                    if (out2) out2[q] = pp;
                    if (c == 2u) {
                        out1[q + 1] = (int)hi;
                        if (out2) out2[q + 1] = pp;
                    }
                } else {
                    const uint32_t a = hi >> 4;
                    for (uint32_t e = 0; e < c; e++) {
                        out1[q + e] = bpos[a + e];
                        if (out2) out2[q + e] = pp;
                    }
                }
            }
        }
        o += tot;
    }
}

// Duplicate keys without a sort (round 3): the build rows are partitioned by window
// like the unique build's (stable, so a window's rows keep their input order), and
// one block per window finds the runs itself. In LDS: its keys go into the window's
// slots by CAS (u32 keys; the key -1, the u32 empty marker, flags), a u16 count per
// slot, one scan over the slots in slot order gives each slot's run its place in
// the window's stretch of the run array, and each row takes a place in its run by
// one atomic; rows of a key arrive at their places in any order, so a row's final
// place is its run's start + the number of the run's rows before it in input order
// (their input indices sit in LDS by place). The row writes its payload there (the
// key's build positions in insertion order, bpos), and the window's table words
// carry {key, start << 4 | length} with the unique build's overflow marks. A window
// of more than kRunRows rows or a key on 15 rows or more (not packable) flags
// *general; the caller then takes the sorted-runs build. Replaces, at 2^28 rows with
// every key twice, the 4-pass sort of the pairs, the run extraction and the
// partition of the distinct keys.
constexpr uint32_t kRunRows = 6144;  // rows a window block takes (3/4 of its slots)
constexpr uint32_t kEmpty32 = ~0u;

__global__ __launch_bounds__(kWinTPB) void k_win_build_runs(const u64* __restrict__ in,
                                                            const uint32_t* __restrict__ wstart,
                                                            u64* __restrict__ words, int* __restrict__ bpos, Win t,
                                                            uint32_t* __restrict__ general) {
    constexpr uint32_t W = 1u << kWinLog;
    constexpr int kPer = (int)(kRunRows / kWinTPB);  // rows per thread
    constexpr int kW = kWinTPB / 64;
    __shared__ uint32_t tab[W];          // keys by slot
    __shared__ uint32_t c32[W / 2];      // u16 per slot: counts, then run places
    __shared__ uint16_t pidx[kRunRows];  // input index (within the window) by place
    __shared__ uint8_t ovf[W / kBucket];
    __shared__ uint32_t wsum[kW + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t w = blockIdx.x;
    const uint32_t b = wstart[w], e = wstart[w + 1], c = e - b;
    if (W != (uint32_t)t.wmask + 1 || c > kRunRows) {  // (a table smaller than one window: never here)
        if (tid == 0) *general = 1;
        return;
    }
    for (uint32_t x = tid; x < W; x += kWinTPB) tab[x] = kEmpty32;
    for (uint32_t x = tid; x < W / 2; x += kWinTPB) c32[x] = 0;
    for (uint32_t x = tid; x < W / kBucket; x += kWinTPB) ovf[x] = 0;
    if (tid == 0) wsum[kW] = 0;
    __syncthreads();
    uint32_t key[kPer], pay[kPer], slot[kPer];
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint32_t i = (uint32_t)k * kWinTPB + tid;
        const u64 v = i < c ? in[b + i] : 0ull;
        key[k] = (uint32_t)v;
        pay[k] = (uint32_t)(v >> 32);
    }
    bool bad = false;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        slot[k] = 0;
        if ((uint32_t)k * kWinTPB + tid >= c) continue;
        if (key[k] == kEmpty32) {
            bad = true;
            continue;
        }
        const uint32_t h0 = (uint32_t)ht_home(key[k], t.wmask);
        uint32_t h = h0;
        for (uint32_t step = 0; step < W; step++) {
            const uint32_t old = atomicCAS(&tab[h], kEmpty32, key[k]);
            if (old == kEmpty32 || old == key[k]) {
                if (old == kEmpty32 && step >= kBucket) ovf[h0 / kBucket] = 1;
                break;
            }
            h = (h + 1) & (W - 1);
        }
        slot[k] = h;
        atomicAdd(&c32[h >> 1], 1u << (16 * (h & 1)));
    }
    if (bad) wsum[kW] = 1;
    __syncthreads();
    // exclusive scan of the counts in slot order: lane-consecutive words, 4 a thread
    constexpr int kQ = (int)(W / 2 / kWinTPB);
    uint32_t* mine = c32 + (uint32_t)tid * kQ;
    uint32_t tot = 0, mx = 0;
#pragma unroll
    for (int j = 0; j < kQ; j++) {
        const uint32_t cell = mine[j], lo = cell & 0xFFFFu, hi = cell >> 16;
        mx = lo > mx ? lo : mx;
        mx = hi > mx ? hi : mx;
        tot += lo + hi;
    }
    uint32_t incl = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(incl, off, 64);
        if (lane >= off) incl += y;
    }
    if (lane == 63) wsum[wave] = incl;
    if (__ballot(mx >= 15u)) wsum[kW] = 1;  // a run the packed payload cannot hold
    __syncthreads();
    if (wsum[kW]) {
        if (tid == 0) *general = 1;
        return;
    }
    uint32_t run = incl - tot;
    for (int v = 0; v < wave; v++) run += wsum[v];
#pragma unroll
    for (int j = 0; j < kQ; j++) {
        const uint32_t cell = mine[j], lo = cell & 0xFFFFu;
        mine[j] = run | ((run + lo) << 16);
        run += lo + (cell >> 16);
    }
    __syncthreads();
    uint32_t place[kPer];
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        place[k] = 0;
        const uint32_t i = (uint32_t)k * kWinTPB + tid;
        if (i >= c) continue;
        const uint32_t h = slot[k], sh = 16 * (h & 1);
        place[k] = (atomicAdd(&c32[h >> 1], 1u << sh) >> sh) & 0xFFFFu;
        pidx[place[k]] = (uint16_t)i;
    }
    __syncthreads();
    // c32 now holds each slot's run end; its run starts where slot h - 1's ends.
    // The window's table words first, a bucket (4 slots) per thread, with the overflow
    // marks; then tab's space stages the payloads by final place, so the run array
    // leaves in one coalesced copy (the rows' own stores were scattered 4-byte writes)
    const uint16_t* c16 = reinterpret_cast<const uint16_t*>(c32);
    u64* dst = words + (uint64_t)w * W;
    for (uint32_t bk = tid; bk < W / kBucket; bk += kWinTPB) {
        u64 o[kBucket];
        bool full = true;
#pragma unroll
        for (uint32_t q = 0; q < kBucket; q++) {
            const uint32_t h = bk * kBucket + q;
            const uint32_t k = tab[h];
            if (k == kEmpty32) {
                o[q] = kEmpty;
                full = false;
            } else {
                const uint32_t s0 = h ? c16[h - 1] : 0u, s1 = c16[h];
                o[q] = (u64)k | ((u64)(((b + s0) << 4) | (s1 - s0)) << 32);
            }
        }
        if (full && (((uint32_t)o[0] > (uint32_t)o[1]) != (ovf[bk] != 0))) {
            const u64 x = o[0];
            o[0] = o[1];
            o[1] = x;
        }
#pragma unroll
        for (uint32_t q = 0; q < kBucket; q++) dst[bk * kBucket + q] = o[q];
    }
    __syncthreads();
    uint32_t* stage = tab;  // (W >= kRunRows)
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint32_t i = (uint32_t)k * kWinTPB + tid;
        if (i >= c) continue;
        const uint32_t h = slot[k];
        const uint32_t s0 = h ? c16[h - 1] : 0u, s1 = c16[h];
        uint32_t r = 0;
        for (uint32_t q = s0; q < s1; q++) r += pidx[q] < i;
        stage[s0 + r] = pay[k];
    }
    __syncthreads();
    for (uint32_t x = tid; x < c; x += kWinTPB) bpos[b + x] = (int)stage[x];
}

// The build's (key, payload) words in a stable LSD radix partition by table window (8 bits
// of the window id a pass). *words = the partitioned words and *wstart = each window's
// first word (*nwin + 1 entries): pool blocks, now the caller's. Everything else the passes
// used is freed in stream order. pmm (when not null): the payloads' range (k_win_scatter).
int partition_by_window(const int* c1, const int* p1, uint64_t n, const Win& t, uint64_t slots, int* pmm,
                        hipStream_t st, u64** words, uint32_t** wstart_out, uint32_t* nwin, int* passes_out) {
    int lg = 0;
    while ((1ull << lg) < slots) lg++;
    const int passes = (lg - t.wlog + 7) / 8;
    const uint32_t nw = (uint32_t)(slots >> t.wlog);
    const uint64_t ntiles = ceil_div(n, (uint64_t)kBTPB * kSortItems);
    const uint64_t nh = ntiles * kRadix;
    u64 *a = nullptr, *b = nullptr, *hscan = nullptr, *scratch = nullptr;
    uint32_t *hist = nullptr, *wstart = nullptr;
    auto done = [&](int rc) {
        pool_free_on(a, st);
        pool_free_on(b, st);
        pool_free_on(hist, st);
        pool_free_on(hscan, st);
        pool_free_on(scratch, st);
        pool_free_on(wstart, st);
        return rc;
    };
    a = (u64*)pool_alloc(n * 8);
    b = passes > 1 ? (u64*)pool_alloc(n * 8) : nullptr;
    hist = (uint32_t*)pool_alloc(nh * 4);
    hscan = (u64*)pool_alloc(nh * 8);
    scratch = (u64*)pool_alloc(scan_u32_scratch_elems(nh) * 8);
    wstart = (uint32_t*)pool_alloc(((uint64_t)nw + 1) * 4);
    if (!a || (passes > 1 && !b) || !hist || !hscan || !scratch || !wstart)
        return done(set_err(MQ_ENOMEM, "join: window partition buffers (%llu rows)", (unsigned long long)n));
    u64* src = nullptr;
    u64* dst = a;
    for (int pass = 0; pass < passes; pass++) {
        const int shift = 8 * pass;
        // (round 6 measured digit bytes for the next pass's histogram, as the index sort
        // writes them: the byte stores cost the scatter 0.2-0.4 ms at 2^28 against the
        // histogram's 0.32 ms saved; not kept)
        if (pass == 0) {
            hipLaunchKernelGGL(k_win_hist<true>, dim3((uint32_t)ntiles), dim3(kBTPB), 0, st, c1,
                               (const u64*)nullptr, n, t, shift, hist, (uint32_t)ntiles);
        } else {
            hipLaunchKernelGGL(k_win_hist<false>, dim3((uint32_t)ntiles), dim3(kBTPB), 0, st,
                               (const int*)nullptr, src, n, t, shift, hist, (uint32_t)ntiles);
        }
        int rc = scan_u32_exclusive(hist, hscan, nh, scratch, st);
        if (rc) return done(rc);
        if (pass == 0) {
            hipLaunchKernelGGL(k_win_scatter<true>, dim3((uint32_t)ntiles), dim3(kBTPB), 0, st, c1, p1,
                               (const u64*)nullptr, n, t, shift, hscan, (uint32_t)ntiles, dst, pmm);
        } else {
            hipLaunchKernelGGL(k_win_scatter<false>, dim3((uint32_t)ntiles), dim3(kBTPB), 0, st,
                               (const int*)nullptr, (const int*)nullptr, src, n, t, shift, hscan,
                               (uint32_t)ntiles, dst, (int*)nullptr);
        }
        if (hipGetLastError() != hipSuccess) return done(set_err(MQ_EHIP, "join: window partition"));
        src = dst;
        dst = (dst == a) ? b : a;
    }
    hipLaunchKernelGGL(k_win_bounds<u64>, dim3(nw / kTPB + 1), dim3(kTPB), 0, st, src, n, t, nw, wstart);
    if (hipGetLastError() != hipSuccess) return done(set_err(MQ_EHIP, "join: window bounds"));
    *words = src;
    *wstart_out = wstart;
    *nwin = nw;
    *passes_out = passes;
    a = dst, b = nullptr, wstart = nullptr;  // (dst: the ping-pong buffer without the result)
    return done(MQ_OK);
}

}  // namespace

namespace mqj {

int win_build_table(mq_join* j, const int* c1, const int* p1, uint64_t n, uint64_t slots, uint32_t* general,
                    hipStream_t st) {
    u64* words = nullptr;
    uint32_t *wstart = nullptr, nw = 0;
    int passes = 0;
    int rc = partition_by_window(c1, p1, n, j->win, slots, nullptr, st, &words, &wstart, &nw, &passes);
    if (rc) return rc;
    hipLaunchKernelGGL(k_win_build, dim3(nw), dim3(kWinTPB), 0, st, words, wstart, j->words, j->win, general);
    if (hipGetLastError() != hipSuccess) rc = set_err(MQ_EHIP, "join: window build");
    // the partition is released only after the build has run
    else if (hipStreamSynchronize(st) != hipSuccess) rc = set_err(MQ_EHIP, "join: build sync");
    pool_free_on(words, st);
    pool_free_on(wstart, st);
    return rc;
}

int win_keep_partition(mq_join* j, const int* c1, const int* p1, uint64_t n, uint64_t slots, int* pmm,
                       hipStream_t st) {
    u64* words = nullptr;
    uint32_t *wstart = nullptr, nw = 0;
    int passes = 0;
    int rc = partition_by_window(c1, p1, n, j->win, slots, pmm, st, &words, &wstart, &nw, &passes);
    if (rc) return rc;
    if ((rc = jown(j, words))) {  // (jown freed words, stream-ordered)
        pool_free_on(wstart, st);
        return rc;
    }
    if ((rc = jown(j, wstart))) return rc;
    j->marks = true;  // (the table a small probe asks for later is k_win_build's)
    j->pwords = words;
    j->pwstart = wstart;
    j->nwin = nw;
    j->passes = passes;
    return MQ_OK;
}

// Duplicate keys, windowed (k_win_build_runs): the build rows partitioned by window
// (the unique build's passes), then each window's runs found in LDS. Returns 0
// (j->unique = 2, packed payloads, j->bpos the runs), 1 when it does not apply or a
// window flagged (the caller takes the sorted-runs build), or an error.
int build_window_runs(mq_join* j, const int* c1, const int* p1, uint64_t n, uint64_t slots, uint32_t* general,
                      hipStream_t st, int* pmm) {
    if (knob_off("MQ_JOIN_WINRUNS") || knob_off("MQ_JOIN_RUNS") || n < kWindowBuildRows || n > (1ull << 28) ||
        j->win.wlog != kWinLog)
        return 1;
    // bp joins the handle only when the build takes this path
    int* bp = (int*)pool_alloc(n * 4);
    u64* words = nullptr;
    uint32_t *wstart = nullptr, nw = 0;
    int passes = 0;
    auto drop = [&](int rc) {  // (stream-ordered: launched work may still use them)
        pool_free_on(bp, st);
        pool_free_on(words, st);
        pool_free_on(wstart, st);
        return rc;
    };
    if (!bp) return drop(set_err(MQ_ENOMEM, "join: window runs outputs (%llu rows)", (unsigned long long)n));
    int rc = partition_by_window(c1, p1, n, j->win, slots, pmm, st, &words, &wstart, &nw, &passes);
    if (rc) return drop(rc);
    uint32_t flag = 0;
    if (hipMemsetAsync(general, 0, 4, st) != hipSuccess) return drop(set_err(MQ_EHIP, "join: memset"));
    hipLaunchKernelGGL(k_win_build_runs, dim3(nw), dim3(kWinTPB), 0, st, words, wstart, j->words, bp, j->win, general);
    if (hipGetLastError() != hipSuccess) return drop(set_err(MQ_EHIP, "join: window runs build"));
    int sl[128];
    if (hipMemcpyAsync(&flag, general, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (pmm && hipMemcpyAsync(sl, pmm, sizeof sl, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
        return drop(set_err(MQ_EHIP, "join: window runs sync"));
    if (flag) return drop(1);
    // a value outside the payloads' range: the partitioned probe's marker (rsent)
    if (pmm) fold_payload_range(j, sl, true);
    int* const bpos = bp;
    bp = nullptr;  // (jown frees it itself when it fails)
    if ((rc = jown(j, bpos))) return drop(rc);
    j->unique = 2;
    j->packed = true;
    j->rs = nullptr;  // packed lengths stay below 15: no run is looked up
    j->bpos = bpos;
    j->marks = true;
    return drop(0);
}

}  // namespace mqj

namespace {

// defer (round 6): the last inverse pass is left to mq_join_write, fused with the pair
// write (k_pwin_gather_write); the handle keeps what it reads: pass 0's places of the
// probe rows, its tile offsets and the results in pass-0 order.
template <typename RT, bool RUNS = false>
int probe_partitioned_t(mq_join* j, const int32_t* d_c2, uint64_t n2, uint32_t* pstart, u64* hits, hipStream_t st,
                        bool defer = false) {
    const Win t = j->win;
    const int passes = j->passes;
    constexpr int PT = probe_tpb<RT>();  // the probe partition's tile width
    const uint64_t ntiles = probe_tiles(n2, PT), nh = ntiles * kRadix;
    uint32_t* K[4] = {reinterpret_cast<uint32_t*>(const_cast<int32_t*>(d_c2)), nullptr, nullptr, nullptr};
    u64* hs[3] = {nullptr, nullptr, nullptr};
    uint16_t* P[3] = {nullptr, nullptr, nullptr};  // each pass's places of its input rows
    RT* R[2] = {nullptr, nullptr};
    uint32_t *hist = nullptr, *pws = nullptr;
    u64* scratch = nullptr;
    auto done = [&](int rc) {
        for (int p = 1; p <= passes; p++) pool_free_on(K[p], st);
        for (int p = 0; p < passes; p++) pool_free_on(hs[p], st);
        for (int p = 0; p < passes; p++) pool_free_on(P[p], st);
        pool_free_on(R[0], st);
        pool_free_on(R[1], st);
        pool_free_on(hist, st);
        pool_free_on(pws, st);
        pool_free_on(scratch, st);
        return rc;
    };
    bool ok = true;
    for (int p = 1; p <= passes; p++) ok = ok && (K[p] = (uint32_t*)pool_alloc(n2 * 4));
    for (int p = 0; p < passes; p++) ok = ok && (hs[p] = (u64*)pool_alloc(nh * 8));
    for (int p = 0; p < passes; p++) ok = ok && (P[p] = (uint16_t*)pool_alloc(n2 * 2));
    ok = ok && (R[0] = (RT*)pool_alloc(n2 * sizeof(RT))) && (passes < 2 || (R[1] = (RT*)pool_alloc(n2 * sizeof(RT)))) &&
         (hist = (uint32_t*)pool_alloc(nh * 4)) && (pws = (uint32_t*)pool_alloc(((uint64_t)j->nwin + 1) * 4)) &&
         (scratch = (u64*)pool_alloc(scan_u32_scratch_elems(nh) * 8));
    if (!ok) return done(set_err(MQ_ENOMEM, "join: partitioned probe buffers (%llu rows)", (unsigned long long)n2));
    for (int p = 0; p < passes; p++) {
        hipLaunchKernelGGL((k_win_hist<true, PT>), dim3((uint32_t)ntiles), dim3(PT), 0, st, (const int*)K[p],
                           (const u64*)nullptr, n2, t, 8 * p, hist, (uint32_t)ntiles);
        int rc = scan_u32_exclusive(hist, hs[p], nh, scratch, st);
        if (rc) return done(rc);
        if (p == 0)  // (the first pass needs no order within a digit)
            hipLaunchKernelGGL((k_pwin_scatter<PT, false>), dim3((uint32_t)ntiles), dim3(PT), 0, st, K[p], n2, t, 8 * p,
                               hs[p], (uint32_t)ntiles, K[p + 1], P[p]);
        else
            hipLaunchKernelGGL((k_pwin_scatter<PT, true>), dim3((uint32_t)ntiles), dim3(PT), 0, st, K[p], n2, t, 8 * p,
                               hs[p], (uint32_t)ntiles, K[p + 1], P[p]);
        if (hipGetLastError() != hipSuccess) return done(set_err(MQ_EHIP, "join: probe partition"));
    }
    hipLaunchKernelGGL(k_win_bounds<uint32_t>, dim3(j->nwin / kTPB + 1), dim3(kTPB), 0, st, K[passes], n2, t,
                       j->nwin, pws);
    DevState* s;
    if (int rc0 = ensure_ready(&s)) return done(rc0);
    const uint32_t gj = j->nwin < (uint32_t)s->cus * 2 ? j->nwin : (uint32_t)s->cus * 2;
    if constexpr (RUNS && sizeof(RT) == 8)  // duplicate keys on the partitioned words (run2 records)
        hipLaunchKernelGGL(k_win_join_runs, dim3(gj), dim3(kWinTPB), 0, st, j->pwords, j->pwstart, K[passes], pws,
                           j->nwin, t, reinterpret_cast<u64*>(R[0]), const_cast<int*>(j->bpos), j->pflag, j->mtot,
                           j->sentinel);
    else if constexpr (RUNS)  // a windowed runs table (k_win_build_runs), a slice per window in LDS
        hipLaunchKernelGGL(k_win_probe_tab<RT>, dim3(gj), dim3(kWinTPB), 0, st, (const u64*)j->words, K[passes], pws,
                           j->nwin, t, R[0]);
    else
        hipLaunchKernelGGL(k_win_join<RT>, dim3(gj), dim3(kWinTPB), 0, st, j->pwords, j->pwstart, K[passes], pws,
                           j->nwin, t, R[0], j->pflag, j->sentinel, j->mtot);
    if (hipGetLastError() != hipSuccess) return done(set_err(MQ_EHIP, "join: window join"));
    int cur = 0;
    for (int p = passes - 1; p >= 0; p--) {
        if (p == 0 && defer) {
            j->pr.dperm = P[0];
            P[0] = nullptr;
            j->pr.dhs0 = hs[0];
            j->pr.dres = R[cur];
            hs[0] = nullptr;
            R[cur] = nullptr;
            j->pr.deferred = true;
            break;
        }
        if (p == 0)
            hipLaunchKernelGGL((k_pwin_gather<true, RT, RUNS, PT>), dim3((uint32_t)ntiles), dim3(PT), 0, st, P[0], n2,
                               hs[0], (uint32_t)ntiles, (const RT*)R[cur], (RT*)(RUNS ? (void*)j->pr.p01 : nullptr),
                               pstart, hits, j->sentinel);
        else
            hipLaunchKernelGGL((k_pwin_gather<false, RT, false, PT>), dim3((uint32_t)ntiles), dim3(PT), 0, st, P[p], n2,
                               hs[p], (uint32_t)ntiles, (const RT*)R[cur], R[cur ^ 1], (uint32_t*)nullptr,
                               (u64*)nullptr, j->sentinel);
        if (hipGetLastError() != hipSuccess) return done(set_err(MQ_EHIP, "join: probe unpartition"));
        cur ^= 1;
    }
    return done(MQ_OK);
}

// A deferred probe's last inverse pass, by the handle's mode: in the classic form (per-row
// results into pstart / p01, hit words or per-word run lengths into hits) ...
void launch_final_gather(mq_join* j, u64* hits, hipStream_t st) {
    const ProbeState& p = j->pr;
    const uint32_t ntiles = (uint32_t)probe_tiles(p.n2, deferred_tpb(p.dmode));
    const dim3 g(ntiles), b(deferred_tpb(p.dmode));
    if (p.dmode == 2)
        hipLaunchKernelGGL((k_pwin_gather<true, u64, true, deferred_tpb(2)>), g, b, 0, st, p.dperm, p.n2, p.dhs0, ntiles,
                           (const u64*)p.dres, p.p01, p.pstart, hits, j->sentinel);
    else if (p.dmode == 1)
        hipLaunchKernelGGL((k_pwin_gather<true, u64, false, deferred_tpb(1)>), g, b, 0, st, p.dperm, p.n2, p.dhs0, ntiles,
                           (const u64*)p.dres, (u64*)nullptr, p.pstart, hits, j->sentinel);
    else
        hipLaunchKernelGGL((k_pwin_gather<true, uint32_t, false, deferred_tpb(0)>), g, b, 0, st, p.dperm, p.n2, p.dhs0,
                           ntiles, (const uint32_t*)p.dres, (uint32_t*)nullptr, p.pstart, hits, j->sentinel);
}

// ... or fused with the pair write (stat: the tiles' look-back status, zeroed).
void launch_gather_write(mq_join* j, const int32_t* d_p2, int32_t* d_out1, int32_t* d_out2, u64* stat,
                         hipStream_t st) {
    const ProbeState& p = j->pr;
    const uint32_t ntiles = (uint32_t)probe_tiles(p.n2, deferred_tpb(p.dmode));
    const dim3 g(ntiles), b(deferred_tpb(p.dmode));
    if (p.dmode == 2)
        hipLaunchKernelGGL((k_pwin_gather_write<u64, 2, deferred_tpb(2)>), g, b, 0, st, p.dperm, p.n2, p.dhs0, ntiles,
                           (const u64*)p.dres, d_p2, j->bpos, j->sentinel, d_out1, d_out2, stat, j->pflag + 1);
    else if (p.dmode == 1)
        hipLaunchKernelGGL((k_pwin_gather_write<u64, 1, deferred_tpb(1)>), g, b, 0, st, p.dperm, p.n2, p.dhs0, ntiles,
                           (const u64*)p.dres, d_p2, j->bpos, j->sentinel, d_out1, d_out2, stat, j->pflag + 1);
    else
        hipLaunchKernelGGL((k_pwin_gather_write<uint32_t, 0, deferred_tpb(0)>), g, b, 0, st, p.dperm, p.n2, p.dhs0,
                           ntiles, (const uint32_t*)p.dres, d_p2, j->bpos, j->sentinel, d_out1, d_out2, stat,
                           j->pflag + 1);
}

}  // namespace

namespace mqj {

int probe_partitioned_deferred(mq_join* j, const int32_t* d_c2, uint64_t n2, hipStream_t st) {
    j->pr.dmode = j->dupw ? 2 : j->narrow ? 0 : 1;
    if (j->dupw) return probe_partitioned_t<u64, true>(j, d_c2, n2, nullptr, nullptr, st, true);
    if (j->narrow) return probe_partitioned_t<uint32_t>(j, d_c2, n2, nullptr, nullptr, st, true);
    return probe_partitioned_t<u64>(j, d_c2, n2, nullptr, nullptr, st, true);
}

// The same over a windowed runs table (j->words, built by k_win_build_runs): per row the
// packed run (pstart) and per 64 rows the run lengths' sum (wcnt).
int probe_partitioned_runs(mq_join* j, const int32_t* d_c2, uint64_t n2, uint32_t* pstart, uint32_t* wcnt,
                           hipStream_t st) {
    int lg = 0;
    while ((1ull << lg) < j->mask + 1) lg++;
    j->nwin = (uint32_t)((j->mask + 1) >> j->win.wlog);
    j->passes = (lg - j->win.wlog + 7) / 8;
    if (j->dupw)  // run2 records from the partitioned build words (j->pr.p01: n2 u64)
        return probe_partitioned_t<u64, true>(j, d_c2, n2, pstart, reinterpret_cast<u64*>(wcnt), st);
    return probe_partitioned_t<uint32_t, true>(j, d_c2, n2, pstart, reinterpret_cast<u64*>(wcnt), st);
}

// A deferred probe's last inverse pass in the classic form (per-row results, hit words or
// per-word run lengths, their scan): for mq_join_counts, whose caller (the key-partitioned
// shard join) needs every row's pair count; mq_join_write then takes the classic kernels.
int finish_classic(mq_join* j, hipStream_t st) {
    DevState* s;
    if (int rc = ensure_ready(&s)) return rc;
    ProbeState& p = j->pr;
    const uint64_t n2 = p.n2, nw = (n2 + 63) / 64;
    const bool runs = p.dmode == 2;
    p.pstart = (uint32_t*)pool_alloc(n2 * 4);
    p.plen = (uint32_t*)pool_alloc(runs ? nw * 4 : nw * 12);
    p.offs = (u64*)pool_alloc(nw * 8);
    p.scan_scratch = (u64*)pool_alloc(scan_u32_scratch_elems(nw) * 8);
    if (runs) p.p01 = (u64*)pool_alloc(n2 * 8);
    if (!p.pstart || !p.plen || !p.offs || !p.scan_scratch || (runs && !p.p01))
        return set_err(MQ_ENOMEM, "mq_join_counts: buffers for %llu rows", (unsigned long long)n2);
    uint32_t* const cnt = runs ? p.plen : p.plen + 2 * nw;
    u64* const hits = reinterpret_cast<u64*>(p.plen);
    launch_final_gather(j, hits, st);
    LAUNCHCHK("k_pwin_gather");
    if (!runs)
        if (int rc = hits_count(s, hits, nw, cnt, st)) return rc;
    if (int rc = scan_u32_exclusive(cnt, p.offs, nw, p.scan_scratch, st)) return rc;
    release_deferred(j, st);
    return MQ_OK;
}

// mq_join_write of a deferred probe: the last inverse pass fused with the pair write
// (look-back over tiles).
int write_deferred(mq_join* j, const int32_t* d_p2, int32_t* d_out1, int32_t* d_out2, hipStream_t st) {
    const uint64_t ntiles = probe_tiles(j->pr.n2, deferred_tpb(j->pr.dmode));
    u64* stat = (u64*)pool_alloc(ntiles * 8 + 16);
    if (!stat) return set_err(MQ_ENOMEM, "mq_join_write: tile status");
    HIPCHK(hipMemsetAsync(stat, 0, ntiles * 8 + 16, st));
    HIPCHK(hipMemsetAsync(j->pflag + 1, 0, 4, st));
    launch_gather_write(j, d_p2, d_out1, d_out2, stat, st);
    const hipError_t e = hipGetLastError();
    pool_free_on(stat, st);
    if (e != hipSuccess) return set_err(MQ_EHIP, "launch of k_pwin_gather_write failed: %s", hipGetErrorString(e));
    return MQ_OK;
}

// The global table of a partitioned build, for a probe too small to pay for its own
// partition (and the handle's later probes): the checked windows stored as k_win_build
// stores them.
// *flagged = 1 when the windows hold a duplicate key, the empty marker or an overfull
// window: the caller then rebuilds without the partition (rebuild_unpartitioned).
int materialize_table(mq_join* j, hipStream_t st, bool* flagged) {
    int rc = jalloc(j, (void**)&j->words, j->slots * 8);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(j->pflag, 0, 4, st));
    hipLaunchKernelGGL(k_win_build, dim3(j->nwin), dim3(kWinTPB), 0, st, j->pwords, j->pwstart, j->words, j->win,
                       j->pflag);
    LAUNCHCHK("k_win_build");
    uint32_t f = 0;
    HIPCHK(hipMemcpyAsync(&f, j->pflag, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *flagged = f != 0;
    jdrop(j, j->pwords);
    jdrop(j, j->pwstart);
    j->pwords = nullptr;
    j->pwstart = nullptr;
    j->part = false;
    return MQ_OK;
}

}  // namespace mqj
