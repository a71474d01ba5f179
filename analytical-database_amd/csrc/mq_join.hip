// mq_join.hip — hash join (src/query.c:652-696 over src/multimap.c) for gfx950.
//
// Output contract (the reference's, verified in SURVEY.md §8(a) row J1): pairs
// (build position, probe position) in probe-major order and, for one probe row,
// in build-insertion order.
//
// Build:
//   * unique keys (the FK case, and config 5): one 64-bit word {key, build
//     position} per slot of an open-addressing table (4-slot buckets, linear
//     probing inside 8192-slot windows, all-ones = empty). Above 2^16 rows the
//     rows are radix-partitioned by window and each window is built in LDS by one
//     block (k_win_build), which also leaves overflow marks in full buckets' slot
//     order. A second sighting of a key, or the empty word, raises a flag.
//   * duplicate keys (a sampled duplicate check decides up front for 2^20 rows and
//     up, else the flag): a stable LSD radix sort of (key, position) makes each
//     key's rows one run in insertion order; the runs' distinct keys go into the
//     same windowed table with the run (start, length) packed as payload.
// Probe: one 32-byte bucket read per probe row; continuations past a full bucket
// ride along in later steps through a per-wave LDS queue. Unique table: a payload
// and one hit word per 64 rows, then a scan of the hit words; runs: each row's
// (start, length), then a scan of the lengths. The write kernels copy the pairs.
// No CPU work per row anywhere; the host reads back only the flags and M.
//
// This file: the global-table, runs and write kernels, the build policy and the C API.
// The window partition and the kernels that work window by window are mq_join_part.hip's
// (called through mq_join_impl.h); the scan is mq_scan.hip's, the sort mq_rsort.hip's.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "mq_common.h"
#include "mq_device.h"
#include "mq_join_impl.h"

namespace {

using namespace mqj;

// Claim (or find) key's slot. Returns slot; *fresh = true if this call claimed it.
__device__ __forceinline__ uint64_t ht_claim(u64* words, uint64_t mask, int key, bool* fresh) {
    const u64 w = pack_key(key);
    uint64_t h = hash32((uint32_t)key) & mask;
    for (uint64_t step = 0; step <= mask; step++) {
        const u64 old = atomicCAS(&words[h], 0ull, w);
        if (old == 0ull) {
            *fresh = true;
            return h;
        }
        if (old == w) {
            *fresh = false;
            return h;
        }
        h = (h + 1) & mask;
    }
    *fresh = false;
    return ~0ull;  // unreachable: the table is at most half full
}

__device__ __forceinline__ uint64_t ht_find(const u64* words, uint64_t mask, int key) {
    const u64 w = pack_key(key);
    uint64_t h = hash32((uint32_t)key) & mask;
    for (uint64_t step = 0; step <= mask; step++) {
        const u64 cur = words[h];
        if (cur == w) return h;
        if (cur == 0ull) return ~0ull;
        h = (h + 1) & mask;
    }
    return ~0ull;
}

// Global-CAS insert (builds below kWindowBuildRows): sets *general on a duplicate
// key, the empty marker, or a full window.
__global__ __launch_bounds__(kTPB) void k_ht_insert_unique(const int* __restrict__ keys,
                                                           const int* __restrict__ pay, uint64_t n,
                                                           u64* words, Win t,
                                                           uint32_t* __restrict__ general) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x; i < n; i += stride) {
        const u64 w = pack_pair(keys[i], pay[i]);
        if (w == kEmpty) {
            *general = 1;
            continue;
        }
        const uint32_t key = (uint32_t)w;
        uint64_t h = ht_home(key, t.mask);
        bool placed = false;
        for (uint64_t step = 0; step <= t.wmask; step++) {
            const u64 old = atomicCAS(&words[h], kEmpty, w);
            if (old == kEmpty) {
                placed = true;
                break;
            }
            if ((uint32_t)old == key) break;  // second sighting of the key
            h = win_next(h, t);
        }
        if (!placed) *general = 1;
    }
}

// 2 probes per thread per step: with whole-bucket loads 2 beat 8 (8.25 vs 8.8 ms at
// 2^28, same box: fewer VGPRs, more waves); with single-slot loads 8 had beaten 1.
constexpr int kProbeILP = 2;
constexpr uint32_t kContCap = 320;  // queued continuations per wave (64 taken + 2 x 128 new fit)

// One probe row's outputs. RUNS: the run start and length (0 = no match), from the
// packed payload or, for a long run (or unpacked), from rs. Unique: the payload (the
// build position), whose hit bit is the caller's.
template <bool RUNS>
__device__ __forceinline__ void probe_emit(uint64_t j, bool hit, uint32_t payload, uint32_t* __restrict__ pstart,
                                           const uint32_t* __restrict__ rs, uint32_t* __restrict__ cnt,
                                           bool packed) {
    if constexpr (RUNS) {
        if (!cnt) {  // packed runs: the payload itself (0 = miss), decoded by the write
            pstart[j] = hit ? payload : 0u;
            return;
        }
        uint32_t a = 0, L = 0;
        if (hit) {
            L = packed ? payload & 15u : 15u;
            a = packed ? payload >> 4 : payload;
            if (L == 15u) {
                L = rs[a + 1] - rs[a];
                a = rs[a];
            }
        }
        pstart[j] = a;
        cnt[j] = L;
    } else {
        pstart[j] = payload;  // (misses store 0: whole lines)
    }
}

// A packed run payload's length (a hit's payload is never 0; 15 = look the run up).
__device__ __forceinline__ uint32_t run_len(uint32_t payload, const uint32_t* __restrict__ rs) {
    const uint32_t L = payload & 15u;
    if (L != 15u) return L;
    const uint32_t r = payload >> 4;
    return rs[r + 1] - rs[r];
}

// kProbeILP probes per thread per step: the keys are loaded coalesced, then all
// their home buckets (4 slots, 32 B, two 16-byte loads) are requested before any
// is examined. Random reads cost per 32-B sector (tools/random_read: a 64-B bucket
// takes 10.4 ms at 2^28 where 32 B take 5.6), so every slot read past the bucket
// costs about as much as the bucket itself; a line is long gone from L2 by the
// time a wave comes back to it. Two things keep those reads rare:
//  * overflow marks (windowed builds): a full bucket's slot order says whether any
//    key homed there lies past it; a miss in a full bucket without one ends there
//    (continuations at load 1/2: 10 % of probes -> 5 %; 8.2 -> 6.8 ms);
//  * the rest are not followed on the spot, where the wave would wait for one
//    dependent read per slot: the row goes to a per-wave queue in LDS, and each
//    step the wave takes up to 64 queued rows and requests their next slot with
//    the new buckets, in the same round trip (an unresolved row is requeued).
// RUNS (duplicate keys as runs, the payload a packed run, see run_payload): per row
// the run's start in pstart and its length in cnt (0 = no match) instead of hit
// words. Row indices and steps are kept as u32 (n2 <= 2^31 rows).
template <bool RUNS>
__global__ __launch_bounds__(kTPB) void k_ht_probe_unique(const int* __restrict__ pkeys, uint64_t n2,
                                                          const u64* __restrict__ words, Win t,
                                                          uint32_t* __restrict__ pstart,
                                                          u64* __restrict__ hits, const uint32_t* __restrict__ rs,
                                                          uint32_t* __restrict__ cnt, bool packed, bool marks,
                                                          uint32_t* __restrict__ wcnt) {
    constexpr uint32_t kB = kBucket;
    auto home = [&](uint32_t key) { return ht_home(key, t.mask); };
    __shared__ uint32_t q_j[kTPB / 64][kContCap], q_h[kTPB / 64][kContCap], q_k[kTPB / 64][kContCap];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* const qj = q_j[wave];
    uint32_t* const qh = q_h[wave];
    uint32_t* const qk = q_k[wave];
    uint32_t nq = 0;  // queued rows (wave-uniform)
    const uint64_t lt = (1ull << lane) - 1;
    const uint64_t stride = (uint64_t)gridDim.x * kTPB * kProbeILP;
    uint64_t j0 = (uint64_t)blockIdx.x * kTPB * kProbeILP + threadIdx.x;
    // the next step's keys are loaded while this step's buckets are in flight;
    // indices are clamped (no branch) so nothing serialises the loads
    uint32_t knext[kProbeILP];
#pragma unroll
    for (int u = 0; u < kProbeILP; u++) {
        const uint64_t j = j0 + (uint64_t)u * kTPB;
        knext[u] = (uint32_t)pkeys[j < n2 ? j : n2 - 1];
    }
    // a queued row: cj, its key ck and ch, the slot it is at as steps from its home
    // slot (kBucket.. W-1); the slot itself is recomputed from the key
    auto cont_slot = [&](uint32_t ck, uint32_t ch) {
        const uint64_t hh = home(ck);
        return (hh & ~t.wmask) | ((hh + ch) & t.wmask);
    };
    // a continuation: row cj at step ch with key ck (lanes < ntake hold one)
    auto cont_resolve = [&](bool has, uint32_t cj, uint32_t ch, uint32_t ck, u64 c) {
        // c: the slot's word. Resolved on the key or an empty slot; otherwise requeued.
        bool again = false;
        if (has) {
            if (c == kEmpty || (uint32_t)c == ck || ch >= t.wmask) {  // (a full window: a miss)
                const bool hit = c != kEmpty && (uint32_t)c == ck;
                const uint32_t payload = hit ? (uint32_t)(c >> 32) : 0u;
                if (RUNS || hit) probe_emit<RUNS>(cj, hit, payload, pstart, rs, cnt, packed);
                if (!RUNS && hit) atomicOr(&hits[cj >> 6], 1ull << (cj & 63));  // word stored in an earlier step
                if (RUNS && wcnt && hit) atomicAdd(&wcnt[cj >> 6], run_len(payload, rs));  // likewise
            } else {
                again = true;
            }
        }
        const u64 am = __ballot(again);
        if (again) {
            const uint32_t at = nq + (uint32_t)__popcll(am & lt);
            qj[at] = cj;
            qh[at] = ch + 1;
            qk[at] = ck;
        }
        nq += (uint32_t)__popcll(am);
    };
    // the loop runs while the wave's first row is in range, so all 64 lanes take
    // every step together (the queue count is per wave)
    for (; j0 - (uint64_t)lane < n2; j0 += stride) {
        uint32_t key[kProbeILP];
        uint64_t h[kProbeILP];
        ulonglong2 b0[kProbeILP], b1[kProbeILP];  // the home bucket, slots 0-1 and 2-3
        // up to 64 queued rows from the back of the queue, their slots requested
        // with this step's buckets
        const uint32_t ntake = nq < 64 ? nq : 64;
        const bool has = (uint32_t)lane < ntake;
        uint32_t cj = 0, ch = 0, ck = 0;
        if (has) {
            const uint32_t e = nq - ntake + (uint32_t)lane;
            cj = qj[e];
            ch = qh[e];
            ck = qk[e];
        }
        nq -= ntake;
        u64 c = 0;
        if (has) c = words[cont_slot(ck, ch)];
#pragma unroll
        for (int u = 0; u < kProbeILP; u++) {
            key[u] = knext[u];
            h[u] = home(key[u]);
            const ulonglong2* q = reinterpret_cast<const ulonglong2*>(words + h[u]);
            b0[u] = q[0];
            b1[u] = q[1];
        }
#pragma unroll
        for (int u = 0; u < kProbeILP; u++) {
            const uint64_t j = j0 + stride + (uint64_t)u * kTPB;
            knext[u] = (uint32_t)pkeys[j < n2 ? j : n2 - 1];
        }
        cont_resolve(has, cj, ch, ck, c);
#pragma unroll
        for (int u = 0; u < kProbeILP; u++) {
            const uint64_t j = j0 + (uint64_t)u * kTPB;
            const u64 sl[4] = {b0[u].x, b0[u].y, b1[u].x, b1[u].y};
            bool hit = false, done = j >= n2;
            uint32_t payload = 0;
#pragma unroll
            for (uint32_t i = 0; i < kB; i++) {
                if (done) break;
                const u64 w = sl[i];
                if (w == kEmpty) done = true;
                else if ((uint32_t)w == key[u]) hit = done = true, payload = (uint32_t)(w >> 32);
            }
            // a full bucket without the key: on along the window, unless its mark
            // says no key homed here went on (j < n2 here)
            const bool defer = !done && !(marks && !bucket_ovf(sl[0], sl[1]));
            const u64 dm = __ballot(defer);
            if (defer) {
                const uint32_t at = nq + (uint32_t)__popcll(dm & lt);
                qj[at] = (uint32_t)j;
                qh[at] = kB;
                qk[at] = key[u];
            }
            nq += (uint32_t)__popcll(dm);
            if (j < n2 && !defer) probe_emit<RUNS>(j, hit, payload, pstart, rs, cnt, packed);
            if (RUNS && wcnt) {
                // packed runs: the word's run lengths, summed over the wave (a deferred
                // row adds its own when it resolves), so no pass re-reads the payloads
                uint32_t L = (j < n2 && !defer && hit) ? run_len(payload, rs) : 0u;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) L += __shfl_xor(L, o, 64);
                if (j < n2 && lane == 0) wcnt[j >> 6] = L;
            }
            if constexpr (!RUNS) {
                // a wave's 64 lanes hold 64 consecutive rows: their hits are one word
                // (a deferred row's bit is set when it resolves)
                const u64 m = __ballot(hit);
                if (j < n2 && lane == 0) hits[j >> 6] = m;
            }
        }
        // keep room for a step's worst case (64 requeued + 64 x kProbeILP new):
        // drain in place when the queue runs long
        while (nq > kContCap - 64 - 64 * kProbeILP) {
            const uint32_t nt = nq < 64 ? nq : 64;
            const bool hs = (uint32_t)lane < nt;
            uint32_t dj = 0, dh = 0, dk = 0;
            u64 dc = 0;
            if (hs) {
                const uint32_t e = nq - nt + (uint32_t)lane;
                dj = qj[e], dh = qh[e], dk = qk[e];
                dc = words[cont_slot(dk, dh)];
            }
            nq -= nt;
            cont_resolve(hs, dj, dh, dk, dc);
        }
    }
    // the queue's rest
    while (nq) {
        const uint32_t nt = nq < 64 ? nq : 64;
        const bool hs = (uint32_t)lane < nt;
        uint32_t dj = 0, dh = 0, dk = 0;
        u64 dc = 0;
        if (hs) {
            const uint32_t e = nq - nt + (uint32_t)lane;
            dj = qj[e], dh = qh[e], dk = qk[e];
            dc = words[cont_slot(dk, dh)];
        }
        nq -= nt;
        cont_resolve(hs, dj, dh, dk, dc);
    }
}

// Unique path, after the probe: matches per 64-row hit word (scanned into the
// words' output offsets), then each matching row j writes its pair at its word's
// offset + the matches below it in the word. Output in ascending j, as J1.
__global__ __launch_bounds__(kTPB) void k_hits_count(const u64* __restrict__ hits, uint64_t nw,
                                                     uint32_t* __restrict__ cnt) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t w = (uint64_t)blockIdx.x * kTPB + threadIdx.x; w < nw; w += stride)
        cnt[w] = (uint32_t)__popcll(hits[w]);
}

__global__ __launch_bounds__(kTPB) void k_join_write_hits(const u64* __restrict__ hits,
                                                          const u64* __restrict__ woffs,
                                                          const uint32_t* __restrict__ pstart,
                                                          const int* __restrict__ p2, uint64_t n2,
                                                          int* __restrict__ out1, int* __restrict__ out2) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t j = (uint64_t)blockIdx.x * kTPB + threadIdx.x; j < n2; j += stride) {
        const u64 m = hits[j >> 6];
        const uint32_t b = (uint32_t)(j & 63);
        if (!((m >> b) & 1)) continue;
        const u64 o = woffs[j >> 6] + (u64)__popcll(m & ((1ull << b) - 1));
        out1[o] = (int)pstart[j];
        if (out2) out2[o] = (p2 ? p2[j] : 0);
    }
}

// The same with 4 rows a lane (round 5): payloads and probe positions read as 16-byte
// loads (p2 and pstart 16-byte aligned; else the 1-row kernel), a lane's hits are 4
// bits of its word, its output slot the word's offset plus the hits below them. The
// 1-row form moved its 3 GB at ~3 TB/s (one 4-byte load per thread and iteration).
__global__ __launch_bounds__(kTPB) void k_join_write_hits4(const u64* __restrict__ hits,
                                                           const u64* __restrict__ woffs,
                                                           const uint32_t* __restrict__ pstart,
                                                           const int* __restrict__ p2, uint64_t n2,
                                                           int* __restrict__ out1, int* __restrict__ out2) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB * 4;
    for (uint64_t j = ((uint64_t)blockIdx.x * kTPB + threadIdx.x) * 4; j < n2; j += stride) {
        const u64 m = hits[j >> 6];
        const uint32_t sh = (uint32_t)(j & 63);
        const uint32_t bits = (uint32_t)(m >> sh) & 0xFu;
        if (!bits) continue;
        u64 o = woffs[j >> 6] + (u64)__popcll(m & ((1ull << sh) - 1));
        uint4 pv;
        int4 qv = make_int4(0, 0, 0, 0);
        if (j + 3 < n2) {
            pv = *reinterpret_cast<const uint4*>(pstart + j);
            if (out2 && p2) qv = *reinterpret_cast<const int4*>(p2 + j);
        } else {
            pv.x = pstart[j];
            pv.y = j + 1 < n2 ? pstart[j + 1] : 0u;
            pv.z = j + 2 < n2 ? pstart[j + 2] : 0u;
            pv.w = 0u;
            if (out2 && p2) {
                qv.x = p2[j];
                qv.y = j + 1 < n2 ? p2[j + 1] : 0;
                qv.z = j + 2 < n2 ? p2[j + 2] : 0;
            }
        }
        const uint32_t pa[4] = {pv.x, pv.y, pv.z, pv.w};
        const int qa[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (bits & (1u << e)) {
                out1[o] = (int)pa[e];
                if (out2) out2[o] = qa[e];
                o++;
            }
    }
}

// Diagnostic: k_ht_probe_unique's memory pattern alone (mq_random_read). Read j
// goes to slot hash32(j) of a 2^k-slot table; 8 reads per lane in flight.
__global__ __launch_bounds__(kTPB) void k_random_read(const u64* __restrict__ t, uint64_t mask, uint64_t n,
                                                      u64* __restrict__ out) {
    u64 acc = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kTPB * kProbeILP;
    for (uint64_t j0 = (uint64_t)blockIdx.x * kTPB * kProbeILP + threadIdx.x; j0 < n; j0 += stride) {
        u64 v[kProbeILP];
#pragma unroll
        for (int u = 0; u < kProbeILP; u++) {
            const uint64_t j = j0 + (uint64_t)u * kTPB;
            v[u] = j < n ? t[hash32((uint32_t)j ^ (uint32_t)(j >> 32)) & mask] : 0;
        }
#pragma unroll
        for (int u = 0; u < kProbeILP; u++) acc ^= v[u];
    }
    if (acc == 0x5EED5EED5EED5EEDull) out[0] = acc;  // keeps the loads; never true for a memset table
}

// sorted keys are (key ^ 0x80000000); a run head claims its slot and stores the start
__global__ __launch_bounds__(kTPB) void k_ht_insert_heads(const uint32_t* __restrict__ skeys,
                                                          uint64_t n, u64* words,
                                                          uint32_t* __restrict__ start,
                                                          uint64_t mask) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x; i < n; i += stride) {
        const uint32_t k = skeys[i];
        if (i == 0 || skeys[i - 1] != k) {
            bool fresh;
            const uint64_t h = ht_claim(words, mask, (int)(k ^ 0x80000000u), &fresh);
            start[h] = (uint32_t)i;
        }
    }
}

__global__ __launch_bounds__(kTPB) void k_ht_set_len(const uint32_t* __restrict__ skeys, uint64_t n,
                                                     const u64* words,
                                                     const uint32_t* __restrict__ start,
                                                     uint32_t* __restrict__ len, uint64_t mask) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x; i < n; i += stride) {
        const uint32_t k = skeys[i];
        if (i == n - 1 || skeys[i + 1] != k) {
            const uint64_t h = ht_find(words, mask, (int)(k ^ 0x80000000u));
            len[h] = (uint32_t)(i + 1 - start[h]);
        }
    }
}

__global__ __launch_bounds__(kTPB) void k_ht_probe(const int* __restrict__ pkeys, uint64_t n2,
                                                   const u64* words,
                                                   const uint32_t* __restrict__ start,
                                                   const uint32_t* __restrict__ len, uint64_t mask,
                                                   uint32_t* __restrict__ pstart,
                                                   uint32_t* __restrict__ plen) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t j = (uint64_t)blockIdx.x * kTPB + threadIdx.x; j < n2; j += stride) {
        const uint64_t h = ht_find(words, mask, pkeys[j]);
        const bool hit = h != ~0ull;
        pstart[j] = hit ? start[h] : 0u;
        plen[j] = hit ? len[h] : 0u;
    }
}

// Per-row runs (the sorted-runs and global-CAS builds). A run longer than kLongRun
// rows (a hot key) is not copied by its one lane: the lane lists it as chunks of
// kLongChunk pairs (entry = row << 32 | chunk) and k_join_write_long copies each chunk
// with a whole block, coalesced. (One lane writing a 2^26-row run alone took the wave
// 2^26 dependent iterations.)
constexpr uint32_t kLongRun = 4096;
constexpr uint32_t kLongChunk = 65536;

__global__ __launch_bounds__(kTPB) void k_join_write(const uint32_t* __restrict__ pstart,
                                                     const uint32_t* __restrict__ plen,
                                                     const u64* __restrict__ offs,
                                                     const int* __restrict__ p2,
                                                     const int* __restrict__ bpos, uint64_t n2,
                                                     int* __restrict__ out1, int* __restrict__ out2,
                                                     u64* __restrict__ longq, uint32_t* __restrict__ nlong) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t j = (uint64_t)blockIdx.x * kTPB + threadIdx.x; j < n2; j += stride) {
        const uint32_t L = plen[j];
        if (!L) continue;
        if (L > kLongRun) {
            const uint32_t nch = (L + kLongChunk - 1) / kLongChunk;
            const uint32_t at = atomicAdd(nlong, nch);
            for (uint32_t c = 0; c < nch; c++) longq[at + c] = (j << 32) | c;
            continue;
        }
        const u64 o = offs[j];
        const uint32_t s = pstart[j];
        const int pp = (p2 ? p2[j] : 0);
        for (uint32_t t = 0; t < L; t++) {
            out1[o + t] = bpos[s + t];
            if (out2) out2[o + t] = pp;
        }
    }
}

// The listed chunks of long runs, one block per chunk (grid-stride over the list,
// whose length k_join_write left in *nlong).
__global__ __launch_bounds__(kTPB) void k_join_write_long(const uint32_t* __restrict__ pstart,
                                                          const uint32_t* __restrict__ plen,
                                                          const u64* __restrict__ offs, const int* __restrict__ p2,
                                                          const int* __restrict__ bpos, const u64* __restrict__ longq,
                                                          const uint32_t* __restrict__ nlong, int* __restrict__ out1,
                                                          int* __restrict__ out2) {
    const uint32_t n = *nlong;
    for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {
        const u64 q = longq[e];
        const uint64_t j = q >> 32;
        const uint32_t c = (uint32_t)q;
        const uint32_t L = plen[j];
        const uint32_t a = c * kLongChunk, b = L - a < kLongChunk ? L : a + kLongChunk;
        const u64 o = offs[j];
        const uint32_t s = pstart[j];
        const int pp = (p2 ? p2[j] : 0);
        for (uint32_t t = a + threadIdx.x; t < b; t += kTPB) {
            out1[o + t] = bpos[s + t];
            if (out2) out2[o + t] = pp;
        }
    }
}

// Packed runs (n1 <= 2^28): the probe stores each row's table payload as it is (0 for
// a miss; a hit's payload is never 0: start << 4 | length with length >= 1, or
// r << 4 | 15 for a long run, whose bounds are rs[r], rs[r + 1]). Then per 64-row word
// the sum of the rows' run lengths, a scan over those n2/64 sums, and the write: each
// wave takes one word, its lanes the word's 64 consecutive rows, and a row's output
// offset is the word's offset plus the lengths of the rows below it (a wave prefix).
// (Was: per row a start and a length from the probe and a scan of n2 lengths into
// 8-byte offsets, 16 B more per probe row written and read again, plus the n2 scan.)
__device__ __forceinline__ void run_decode(uint32_t pk, const uint32_t* __restrict__ rs, uint32_t* a, uint32_t* L) {
    uint32_t l = pk & 15u, s = pk >> 4;
    if (l == 15u) {
        l = rs[s + 1] - rs[s];
        s = rs[s];
    }
    *a = pk ? s : 0u;
    *L = pk ? l : 0u;
}

// The packed-runs write (a wave's 64 rows = one word; a row's offset = the word's + a
// wave prefix of the lengths), with more reads in flight: a wave takes kWriteWords words
// at a time (2^28 many-to-many, alternating on one box: 1 word 4.30, 4 words 4.00 ms; on
// another 1 / 4 / 8 words 3.63-4.24 / 3.65-4.03 / 3.58-3.94 ms), and every row's first
// two run positions (all of config 5's runs) are requested for
// all of them before any pair is stored; longer runs finish in a loop. The run reads
// are random (one line of the key-sorted positions per hit row), so the kernel is
// bound by how many of them are outstanding.
template <int kWriteWords>
__global__ __launch_bounds__(kTPB) void k_join_write_runs_mlp(const uint32_t* __restrict__ pk, uint64_t n2,
                                                              const uint32_t* __restrict__ rs,
                                                              const u64* __restrict__ woffs,
                                                              const int* __restrict__ p2,
                                                              const int* __restrict__ bpos, int* __restrict__ out1,
                                                              int* __restrict__ out2) {
    const int lane = threadIdx.x & 63;
    const uint64_t nw = (n2 + 63) / 64;
    const uint64_t wstride = (uint64_t)gridDim.x * (kTPB / 64) * kWriteWords;
    for (uint64_t w0 = ((uint64_t)blockIdx.x * (kTPB / 64) + (threadIdx.x >> 6)) * kWriteWords; w0 < nw;
         w0 += wstride) {
        uint32_t pv[kWriteWords], a[kWriteWords], L[kWriteWords];
        u64 o[kWriteWords];
        int pp[kWriteWords], b0[kWriteWords], b1[kWriteWords];
#pragma unroll
        for (int u = 0; u < kWriteWords; u++) {
            const uint64_t j = (w0 + u) * 64 + (uint64_t)lane;
            pv[u] = j < n2 ? pk[j] : 0u;
            pp[u] = j < n2 ? (p2 ? p2[j] : 0) : 0;
        }
#pragma unroll
        for (int u = 0; u < kWriteWords; u++) {
            run_decode(pv[u], rs, &a[u], &L[u]);
            uint32_t incl = L[u];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t y = __shfl_up(incl, d, 64);
                if (lane >= d) incl += y;
            }
            o[u] = (w0 + u < nw ? woffs[w0 + u] : 0ull) + (u64)(incl - L[u]);
        }
#pragma unroll
        for (int u = 0; u < kWriteWords; u++) {
            b0[u] = L[u] ? bpos[a[u]] : 0;
            b1[u] = L[u] > 1u ? bpos[a[u] + 1] : 0;
        }
#pragma unroll
        for (int u = 0; u < kWriteWords; u++) {
            if (!L[u]) continue;
            out1[o[u]] = b0[u];
            if (out2) out2[o[u]] = pp[u];
            if (L[u] > 1u) {
                out1[o[u] + 1] = b1[u];
                if (out2) out2[o[u] + 1] = pp[u];
            }
            for (uint32_t t = 2; t < L[u]; t++) {
                out1[o[u] + t] = bpos[a[u] + t];
                if (out2) out2[o[u] + t] = pp[u];
            }
        }
    }
}

// The write after a run2 probe (the partitioned runs probe, k_win_probe_tab<u64>): a run
// of one or two rows comes from the probe's per-row positions (p01, a stream), a longer
// one (3..14 rows) from the run array as before.
template <int kWriteWords>
__global__ __launch_bounds__(kTPB) void k_join_write_runs16(const uint32_t* __restrict__ pk, uint64_t n2,
                                                            const u64* __restrict__ woffs, const int* __restrict__ p2,
                                                            const u64* __restrict__ p01, const int* __restrict__ bpos,
                                                            int* __restrict__ out1, int* __restrict__ out2) {
    const int lane = threadIdx.x & 63;
    const uint64_t nw = (n2 + 63) / 64;
    const uint64_t wstride = (uint64_t)gridDim.x * (kTPB / 64) * kWriteWords;
    for (uint64_t w0 = ((uint64_t)blockIdx.x * (kTPB / 64) + (threadIdx.x >> 6)) * kWriteWords; w0 < nw;
         w0 += wstride) {
        uint32_t L[kWriteWords], a[kWriteWords];
        u64 o[kWriteWords], pq[kWriteWords];
        int pp[kWriteWords];
#pragma unroll
        for (int u = 0; u < kWriteWords; u++) {
            const uint64_t j = (w0 + u) * 64 + (uint64_t)lane;
            const uint32_t m = j < n2 ? pk[j] : 0u;
            pq[u] = j < n2 ? p01[j] : 0ull;
            pp[u] = j < n2 ? (p2 ? p2[j] : 0) : 0;
            L[u] = m & 15u;
            a[u] = m >> 4;
        }
#pragma unroll
        for (int u = 0; u < kWriteWords; u++) {
            uint32_t incl = L[u];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t y = __shfl_up(incl, d, 64);
                if (lane >= d) incl += y;
            }
            o[u] = (w0 + u < nw ? woffs[w0 + u] : 0ull) + (u64)(incl - L[u]);
        }
#pragma unroll
        for (int u = 0; u < kWriteWords; u++) {
            if (!L[u]) continue;
            if (L[u] <= 2u) {
                out1[o[u]] = (int)(uint32_t)pq[u];
                if (out2) out2[o[u]] = pp[u];
                if (L[u] == 2u) {
                    out1[o[u] + 1] = (int)(uint32_t)(pq[u] >> 32);
                    if (out2) out2[o[u] + 1] = pp[u];
                }
            } else {
                for (uint32_t t = 0; t < L[u]; t++) {
                    out1[o[u] + t] = bpos[a[u] + t];
                    if (out2) out2[o[u] + t] = pp[u];
                }
            }
        }
    }
}

// ---- duplicate keys as runs (the build sorted by key, stable: a key's rows are one
// run in insertion order); the distinct keys go into the windowed unique table with
// their run index as payload ----
// Runs of the key-sorted build in two passes over the keys: k_run_count counts the
// run heads (a row whose key differs from the row before) per 4096-row tile, an
// exclusive scan of those counts gives each tile its first run, and k_run_emit
// ranks the heads inside the tile (each thread 16 consecutive rows, a block scan of
// the per-thread counts) and writes run r's key dk[r] (unflipped) and first sorted
// row rs[r]; rs[R] = n. k_run_payload then gives every run its payload rid[r]. (Was: a head flag per row, a scan of
// 2^28 flags into 8-byte ranks and a compaction: ≈ 10 GB of traffic, 2.2 ms.)
constexpr int kRunPer = 16;
constexpr uint64_t kRunTile = (uint64_t)kTPB * kRunPer;  // 4096

__device__ __forceinline__ uint32_t run_heads16(const uint32_t* __restrict__ skeys, uint64_t n, uint64_t i0,
                                                uint32_t (&k)[kRunPer]) {
    // bit m set <=> row i0 + m (< n) starts a run; k[] = the 16 keys
    uint32_t prev = i0 ? skeys[i0 - 1] : 0u, bits = 0;
    if (i0 + kRunPer <= n) {
        const uint4* q = reinterpret_cast<const uint4*>(skeys + i0);
#pragma unroll
        for (int v = 0; v < kRunPer / 4; v++) {
            const uint4 x = q[v];
            k[4 * v] = x.x, k[4 * v + 1] = x.y, k[4 * v + 2] = x.z, k[4 * v + 3] = x.w;
        }
    } else {
#pragma unroll
        for (int m = 0; m < kRunPer; m++) k[m] = i0 + m < n ? skeys[i0 + m] : 0u;
    }
#pragma unroll
    for (int m = 0; m < kRunPer; m++) {
        if (i0 + m < n && (i0 + m == 0 || k[m] != prev)) bits |= 1u << m;
        prev = k[m];
    }
    return bits;
}

__global__ __launch_bounds__(kTPB) void k_run_count(const uint32_t* __restrict__ skeys, uint64_t n,
                                                    uint32_t* __restrict__ tcount) {
    __shared__ uint32_t s_w[kTPB / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * kRunTile + (uint64_t)threadIdx.x * kRunPer;
    uint32_t k[kRunPer];
    uint32_t c = i0 < n ? (uint32_t)__popc(run_heads16(skeys, n, i0, k)) : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kTPB / 64; w++) t += s_w[w];
        tcount[blockIdx.x] = t;
    }
}

// (the heads go through LDS: written straight from the ranks, a wave's stores
// scattered over ~2 KB, the emit took 1.03 ms at 2^28)
__global__ __launch_bounds__(kTPB) void k_run_emit(const uint32_t* __restrict__ skeys, uint64_t n,
                                                   const u64* __restrict__ toff, int* __restrict__ dk,
                                                   uint32_t* __restrict__ rs) {
    __shared__ uint32_t s_w[kTPB / 64];
    __shared__ uint32_t s_dk[kRunTile], s_rs[kRunTile];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t i0 = (uint64_t)blockIdx.x * kRunTile + (uint64_t)threadIdx.x * kRunPer;
    uint32_t k[kRunPer];
    const uint32_t bits = i0 < n ? run_heads16(skeys, n, i0, k) : 0u;
    const uint32_t c = (uint32_t)__popc(bits);
    uint32_t incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t at = incl - c, tot = 0;
    for (int w = 0; w < kTPB / 64; w++) {
        if (w < wave) at += s_w[w];
        tot += s_w[w];
    }
#pragma unroll
    for (int m = 0; m < kRunPer; m++) {
        if (bits & (1u << m)) {
            s_dk[at] = k[m] ^ 0x80000000u;
            s_rs[at] = (uint32_t)(i0 + m);
            at++;
        }
    }
    __syncthreads();
    const u64 r0 = toff[blockIdx.x];
    for (uint32_t x = threadIdx.x; x < tot; x += kTPB) {
        dk[r0 + x] = (int)s_dk[x];
        rs[r0 + x] = s_rs[x];
    }
    if (i0 < n && n - i0 <= (uint64_t)kRunPer) rs[r0 + tot] = (uint32_t)n;  // the block holding row n-1
}

// The table payload of run r: (start << 4) | length for runs shorter than 15 rows
// (one probe then yields both), (r << 4) | 15 otherwise (the probe reads rs). Packed
// only while starts and run indexes fit 28 bits (n <= 2^28), else always via rs.
__global__ __launch_bounds__(kTPB) void k_run_payload(const uint32_t* __restrict__ rs, uint64_t R, bool packed,
                                                      int* __restrict__ rid) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t r = (uint64_t)blockIdx.x * kTPB + threadIdx.x; r < R; r += stride) {
        const uint32_t a = rs[r], L = rs[r + 1] - a;
        rid[r] = (int)(!packed ? (uint32_t)r : L < 15u ? (a << 4) | L : ((uint32_t)r << 4) | 15u);
    }
}

// Per probe row, the number of pairs the last probe found for it (mq_join_counts),
// from whichever per-row state the probe left: the unique table's hit words (0/1), a
// packed payload per row (its length, < 15 on the per-word path), or a length per row.
__global__ __launch_bounds__(kTPB) void k_join_counts(const u64* __restrict__ hits, const uint32_t* __restrict__ pk,
                                                      const uint32_t* __restrict__ plen, uint64_t n2,
                                                      uint32_t* __restrict__ cnt) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t j = (uint64_t)blockIdx.x * kTPB + threadIdx.x; j < n2; j += stride) {
        uint32_t c;
        if (hits) c = (uint32_t)(hits[j >> 6] >> (j & 63)) & 1u;
        else if (pk) c = pk[j] & 15u;
        else c = plen[j];
        cnt[j] = c;
    }
}

}  // namespace

namespace mqj {

int jown(mq_join* j, void* p) {
    if (j->nowned >= (int)(sizeof(j->owned) / sizeof(j->owned[0]))) {
        pool_free_on(p, j->stream);  // (stream-ordered: queued work may still write it)
        return set_err(MQ_EINVAL, "join: handle owns too many allocations");
    }
    j->owned[j->nowned++] = p;
    return MQ_OK;
}

int jalloc(mq_join* j, void** p, size_t bytes) {
    *p = pool_alloc(bytes);
    if (!*p) return set_err(MQ_ENOMEM, "join: device allocation of %zu bytes failed", bytes);
    const int rc = jown(j, *p);
    if (rc) *p = nullptr;
    return rc;
}

// Give one owned allocation back (stream-ordered).
void jdrop(mq_join* j, void* p) {
    for (int i = 0; i < j->nowned; i++)
        if (j->owned[i] == p) {
            j->owned[i] = j->owned[--j->nowned];
            pool_free_on(p, j->stream);
            return;
        }
}

int hits_count(const DevState* s, const u64* hits, uint64_t nw, uint32_t* cnt, hipStream_t st) {
    hipLaunchKernelGGL(k_hits_count, dim3(stream_grid(s, nw)), dim3(kTPB), 0, st, hits, nw, cnt);
    LAUNCHCHK("k_hits_count");
    return MQ_OK;
}

void fold_payload_range(mq_join* j, const int (&sl)[128], bool narrow_gates_rsent) {
    int mn = INT32_MAX, mx = INT32_MIN;
    for (int q = 0; q < 64; q++) {
        mn = sl[q] < mn ? sl[q] : mn;
        mx = sl[64 + q] > mx ? sl[64 + q] : mx;
    }
    const bool free_value = mx < INT32_MAX || mn > INT32_MIN;
    const bool narrow_on = !knob_off("MQ_JOIN_NARROW");
    j->sentinel = (uint32_t)(mx < INT32_MAX ? INT32_MAX : INT32_MIN);
    j->rsent_ok = free_value && (narrow_on || !narrow_gates_rsent);
    if (!narrow_gates_rsent) j->narrow = narrow_on && free_value;
}

}  // namespace mqj

namespace {

// Every call queues its work on the stream it is given; one on a different stream than
// the last first waits for that stream, so the handle's queued work is always ordered
// on j->stream and the stream-ordered frees below (pool_free_on) cover all of it: no
// host sync, and shard workers sharing a device do not wait for each other.
int juse(mq_join* j, hipStream_t st) {
    if (j->stream != st) HIPCHK(hipStreamSynchronize(j->stream));
    j->stream = st;
    return MQ_OK;
}

void jfree_all(mq_join* j) {
    for (int i = 0; i < j->nowned; i++) pool_free_on(j->owned[i], j->stream);
    j->nowned = 0;
}

// The partitioned probe from this many build rows (MQ_JOIN_PART_MIN; MQ_JOIN_PART=0: off).
uint64_t part_min_rows() { return knob_off("MQ_JOIN_PART") ? ~0ull : knob_u64("MQ_JOIN_PART_MIN", 1ull << 20); }

// A probe of fewer rows than this takes the global table, not its own partition (its
// passes and the window join read all n1 build words).
uint64_t small_probe_rows(const mq_join* j) {
    const uint64_t pdiv = knob_u64("MQ_JOIN_PART_DIV", 16);
    return j->n1 / (pdiv ? pdiv : 1);
}

// Duplicate keys in a strided sample of the build side (a CAS set of the sampled
// keys): when the sample already has one, the build has many and goes straight to
// the runs build instead of attempting (and abandoning) the unique table.
__global__ __launch_bounds__(kTPB) void k_sample_dups(const int* __restrict__ keys, uint64_t stride, uint32_t ns,
                                                      u64* tab, uint32_t tmask, uint32_t* __restrict__ flag) {
    for (uint32_t i = blockIdx.x * kTPB + threadIdx.x; i < ns; i += gridDim.x * kTPB) {
        const uint32_t key = (uint32_t)keys[(uint64_t)i * stride];
        const u64 w = (u64)key | (1ull << 32);
        uint32_t h = hash32(key) & tmask;
        for (uint32_t step = 0; step <= tmask; step++) {
            const u64 old = atomicCAS(&tab[h], 0ull, w);
            if (old == 0) break;
            if (old == w) {
                *flag = 1;
                break;
            }
            h = (h + 1) & tmask;
        }
    }
}

// 1 when a sample of the build keys holds a duplicate (builds of 2^20 rows and up;
// MQ_JOIN_SAMPLE=0 turns the check off)
int sample_has_dups(const int* c1, uint64_t n, uint32_t* dflag, hipStream_t st, const DevState* s, bool* dups) {
    *dups = false;
    if (n < (1ull << 20) || knob_off("MQ_JOIN_SAMPLE")) return MQ_OK;
    constexpr uint32_t kSample = 1u << 18;
    u64* tab = (u64*)pool_alloc((size_t)2 * kSample * 8);
    if (!tab) return set_err(MQ_ENOMEM, "join: sample set");
    HIPCHK(hipMemsetAsync(tab, 0, (size_t)2 * kSample * 8, st));
    HIPCHK(hipMemsetAsync(dflag + 1, 0, 4, st));
    hipLaunchKernelGGL(k_sample_dups, dim3(stream_grid(s, kSample)), dim3(kTPB), 0, st, c1, n / kSample, kSample, tab,
                       2 * kSample - 1, dflag + 1);
    if (hipGetLastError() != hipSuccess) {
        pool_free_on(tab, st);
        return set_err(MQ_EHIP, "join: sample launch");
    }
    uint32_t f = 0;
    HIPCHK(hipMemcpyAsync(&f, dflag + 1, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    pool_free_on(tab, st);
    *dups = f != 0;
    return MQ_OK;
}

// The unique table into j->words (kWindowBuildRows, mq_join_impl.h): *general is set by a
// duplicate key, the empty word or a full window.
int insert_unique(mq_join* j, const int* c1, const int* p1, uint64_t n, uint64_t slots, uint32_t* general,
                  hipStream_t st, const DevState* s) {
    j->marks = n >= kWindowBuildRows;
    if (j->marks) return win_build_table(j, c1, p1, n, slots, general, st);
    HIPCHK(hipMemsetAsync(j->words, 0xFF, slots * 8, st));
    hipLaunchKernelGGL(k_ht_insert_unique, dim3(stream_grid(s, n)), dim3(kTPB), 0, st, c1, p1, n, j->words, j->win,
                       general);
    LAUNCHCHK("k_ht_insert_unique");
    return MQ_OK;
}

// Duplicate keys: runs of the sorted build, their distinct keys into the windowed
// unique table (payload: run index). Returns 0 (j->unique = 2), 1 when the windowed
// build flagged (the caller takes the global-CAS run table), or an error.
int build_runs(mq_join* j, const uint32_t* skeys, uint64_t n, uint64_t slots, uint32_t* dflag, hipStream_t st,
               const DevState* s) {
    if (knob_off("MQ_JOIN_RUNS")) return 1;  // the global-CAS run table (A/B, tests)
    const uint64_t ntiles = ceil_div(n, kRunTile);
    uint32_t* tcount = (uint32_t*)pool_alloc(ntiles * 4);
    u64* toff = (u64*)pool_alloc(ntiles * 8);
    u64* scratch = (u64*)pool_alloc(scan_u32_scratch_elems(ntiles) * 8);
    auto fail = [&](int rc) {
        pool_free_on(tcount, st);
        pool_free_on(toff, st);
        pool_free_on(scratch, st);
        return rc;
    };
    if (!tcount || !toff || !scratch) return fail(set_err(MQ_ENOMEM, "join: run buffers"));
    hipLaunchKernelGGL(k_run_count, dim3((uint32_t)ntiles), dim3(kTPB), 0, st, skeys, n, tcount);
    int rc = scan_u32_exclusive(tcount, toff, ntiles, scratch, st);
    if (rc) return fail(rc);
    u64 last = 0;
    uint32_t lastc = 0;
    HIPCHK(hipMemcpyAsync(&last, toff + (ntiles - 1), 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&lastc, tcount + (ntiles - 1), 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t R = last + lastc;
    int* dk = (int*)pool_alloc(R * 4);
    int* rid = (int*)pool_alloc(R * 4);
    uint32_t* rs = nullptr;
    if (!dk || !rid || (rc = jalloc(j, (void**)&rs, (R + 1) * 4))) {
        pool_free_on(dk, st);
        pool_free_on(rid, st);
        return fail(rc ? rc : set_err(MQ_ENOMEM, "join: run keys"));
    }
    hipLaunchKernelGGL(k_run_emit, dim3((uint32_t)ntiles), dim3(kTPB), 0, st, skeys, n, toff, dk, rs);
    hipLaunchKernelGGL(k_run_payload, dim3(stream_grid(s, R)), dim3(kTPB), 0, st, rs, R, n <= (1ull << 28), rid);
    if (hipGetLastError() != hipSuccess) rc = set_err(MQ_EHIP, "join: run compaction");
    uint32_t flag = 0;
    if (!rc) HIPCHK(hipMemsetAsync(dflag, 0, 4, st));
    if (!rc) rc = insert_unique(j, dk, rid, R, slots, dflag, st, s);
    if (!rc) {
        HIPCHK(hipMemcpyAsync(&flag, dflag, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    pool_free_on(dk, st);
    pool_free_on(rid, st);
    if (rc) return fail(rc);
    fail(0);
    if (flag) return 1;
    j->unique = 2;
    j->rs = rs;
    j->packed = n <= (1ull << 28);
    return 0;
}

// The duplicate-key window join on the partitioned words (k_win_join_runs) unless a
// test forces one of the runs tables (MQ_JOIN_WINRUNS=0, MQ_JOIN_RUNS=0, MQ_JOIN_RUN2=0)
bool dupw_allowed() {
    return !knob_off("MQ_JOIN_WINRUNS") && !knob_off("MQ_JOIN_RUNS") && !knob_off("MQ_JOIN_RUN2");
}

// A partitioned build (pwords, pwstart kept) turned into the duplicate-key form: packed
// run2 records, long runs' positions into bpos (n1 ints, written by the probe's windows).
int make_dupw(mq_join* j) {
    int* bp = nullptr;
    if (int rc = jalloc(j, (void**)&bp, (j->n1 ? j->n1 : 1) * 4)) return rc;
    j->bpos = bp;
    j->dupw = true;
    j->unique = 2;
    j->packed = true;
    j->rs = nullptr;
    j->marks = true;
    return MQ_OK;
}

// The build proper into a fresh handle (device and stream set). allow_part: a unique
// build of part_min_rows() rows and more keeps its window partition for the
// partitioned probe instead of building the table (a duplicate key or an overfull
// window found there later sends it back here with allow_part = false).
int build_into(mq_join* j, const int32_t* d_c1, const int32_t* d_p1, uint64_t n1, hipStream_t st, DevState* s,
               bool allow_part) {
    int rc;
    j->n1 = n1;
    j->c1 = d_c1;
    j->p1 = d_p1;
    uint64_t slots = 64;
    while (slots < 2 * n1) slots <<= 1;
    j->mask = slots - 1;
    j->win.mask = j->mask;
    j->win.wlog = 0;
    while (j->win.wlog < kWinLog && (1ull << (j->win.wlog + 1)) <= slots) j->win.wlog++;
    j->win.wmask = (1ull << j->win.wlog) - 1;
    j->slots = slots;
    // the partitioned build keeps no global table: allocated only if a path needs it
    const bool part = allow_part && n1 >= kWindowBuildRows && n1 >= part_min_rows() && j->win.wlog == kWinLog;
    uint32_t* dflag = nullptr;
    if ((!part && (rc = jalloc(j, (void**)&j->words, slots * 8))) || (rc = jalloc(j, (void**)&dflag, 16 + 512 + 16)))
        return rc;
    j->pflag = dflag + 2;  // (dflag[1] is the sampled duplicate check's)
    j->mtot = reinterpret_cast<unsigned long long*>(dflag + 132);  // (after the 128 range slots)
    j->bpos = nullptr;  // unique table carries the build positions itself
    j->unique = 1;
    if (n1) {
        HIPCHK(hipMemsetAsync(dflag, 0, 16, st));
        int* pmm = reinterpret_cast<int*>(dflag + 4);  // the payloads' range: 64 min, 64 max slots
        if (part) {  // (bounds at least as wide as the range: 0x7F7F7F7F / 0x80808080 start)
            HIPCHK(hipMemsetAsync(pmm, 0x7F, 64 * 4, st));
            HIPCHK(hipMemsetAsync(pmm + 64, 0x80, 64 * 4, st));
        }
        bool sampled = false;
        if ((rc = sample_has_dups(d_c1, n1, dflag, st, s, &sampled))) return rc;
        uint32_t dup = sampled ? 1u : 0u;
        // the partition alone when the probe will join window by window: unique keys, or
        // (round 6) sampled duplicates answered by k_win_join_runs
        const bool keep = part && (!sampled || dupw_allowed());
        if (keep) {
            if ((rc = win_keep_partition(j, d_c1, d_p1, n1, slots, pmm, st))) return rc;
            // the payloads' range: a value outside it marks a miss (u32 results; the run2
            // records of duplicate keys need one)
            int sl[128];
            HIPCHK(hipMemcpyAsync(sl, pmm, sizeof sl, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            fold_payload_range(j, sl, false);
            j->part = true;
            if (!sampled) return MQ_OK;
            if (j->rsent_ok) return make_dupw(j);
            // duplicates but no free payload value: the runs tables below, from the inputs
            jdrop(j, j->pwords);
            jdrop(j, j->pwstart);
            j->pwords = nullptr;
            j->pwstart = nullptr;
            j->part = false;
        }
        if (!sampled) {
            if ((rc = insert_unique(j, d_c1, d_p1, n1, slots, dflag, st, s))) return rc;
            HIPCHK(hipMemcpyAsync(&dup, dflag, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        if (part && (rc = jalloc(j, (void**)&j->words, slots * 8))) return rc;  // (sampled duplicates)
        if (dup) {  // the payloads' range for the runs probe's marker (the unique attempt's, if any, is spent)
            HIPCHK(hipMemsetAsync(pmm, 0x7F, 64 * 4, st));
            HIPCHK(hipMemsetAsync(pmm + 64, 0x80, 64 * 4, st));
        }
        if (dup && (rc = build_window_runs(j, d_c1, d_p1, n1, slots, dflag, st, pmm)) != 1)
            return rc;  // 0: the windowed runs build took it
        if (dup) {  // general path: stable sort by key, runs in insertion order
            j->unique = 0;
            j->bpos = d_p1;
            uint32_t *skeys, *svals;
            if ((rc = radix_sort_pairs(d_c1, d_p1, n1, &skeys, &svals, st, s))) return rc;
            if ((rc = jown(j, skeys)) || (rc = jown(j, svals))) {
                if (rc && j->owned[j->nowned - 1] != skeys) pool_free_on(svals, st);  // (skeys refused: svals still ours)
                return rc;
            }
            j->bpos = reinterpret_cast<const int*>(svals);
            if ((rc = build_runs(j, skeys, n1, slots, dflag, st, s)) != 1) return rc;  // 0: done, else an error
            // a window of the distinct keys overflowed: the global-CAS table of run heads
            j->unique = 0;
            if ((rc = jalloc(j, (void**)&j->start, slots * 4)) || (rc = jalloc(j, (void**)&j->len, slots * 4)))
                return rc;
            HIPCHK(hipMemsetAsync(j->words, 0, slots * 8, st));
            hipLaunchKernelGGL(k_ht_insert_heads, dim3(stream_grid(s, n1)), dim3(kTPB), 0, st, skeys,
                               n1, j->words, j->start, j->mask);
            LAUNCHCHK("k_ht_insert_heads");
            hipLaunchKernelGGL(k_ht_set_len, dim3(stream_grid(s, n1)), dim3(kTPB), 0, st, skeys, n1,
                               j->words, j->start, j->len, j->mask);
            LAUNCHCHK("k_ht_set_len");
        }
    }
    return MQ_OK;
}

// A partitioned build whose windows turned out to hold a duplicate key (or an overfull
// window, or the table's empty word): everything of the build dropped (stream-ordered)
// and built again from the inputs the old way. The probe arrays stay.
int rebuild_unpartitioned(mq_join* j, hipStream_t st) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    jfree_all(j);
    const int32_t *c1 = j->c1, *p1 = j->p1;
    const uint64_t n1 = j->n1;
    const int device = j->device;
    const ProbeState pr = j->pr;  // (a deferred probe's arrays are freed by the probe that follows)
    std::memset(j, 0, sizeof(*j));
    j->device = device;
    j->stream = st;
    j->pr = pr;
    return build_into(j, c1, p1, n1, st, s, false);
}

// The global-table probe of a windowed table (j->unique 1 or 2), by the handle's form:
//  * unique keys: each row's payload and a hit word per 64 rows (plen), whose popcounts
//    go to cnt;
//  * packed runs of < 15 rows (j->pr.pruns): each row's payload, the per-word run lengths
//    in cnt;
//  * other runs: each row's run start and length (cnt) straight from the probe.
template <bool RUNS>
int launch_probe_unique(const DevState* s, const mq_join* j, const int32_t* d_c2, uint64_t n2, u64* hits,
                        uint32_t* cnt, uint32_t* wcnt, hipStream_t st) {
    auto kern = k_ht_probe_unique<RUNS>;
    hipLaunchKernelGGL(kern, dim3(resident_grid(s, (n2 + kProbeILP - 1) / kProbeILP, (const void*)kern)), dim3(kTPB),
                       0, st, d_c2, n2, j->words, j->win, j->pr.pstart, hits, RUNS ? j->rs : nullptr, cnt,
                       RUNS && j->packed, j->marks, wcnt);
    LAUNCHCHK("k_ht_probe_unique");
    return MQ_OK;
}

int probe_table(const DevState* s, const mq_join* j, const int32_t* d_c2, uint64_t n2, uint32_t* cnt,
                hipStream_t st) {
    if (j->pr.pruns) return launch_probe_unique<true>(s, j, d_c2, n2, nullptr, nullptr, cnt, st);
    if (j->unique == 2) return launch_probe_unique<true>(s, j, d_c2, n2, nullptr, cnt, nullptr, st);
    u64* const hits = reinterpret_cast<u64*>(j->pr.plen);
    if (int rc = launch_probe_unique<false>(s, j, d_c2, n2, hits, nullptr, nullptr, st)) return rc;
    return hits_count(s, hits, (n2 + 63) / 64, cnt, st);
}

}  // namespace

extern "C" {

int mq_join_build(const int32_t* d_c1, const int32_t* d_p1, uint64_t n1, mq_join** out,
                  void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!out || (n1 && (!d_c1 || !d_p1))) return set_err(MQ_EINVAL, "mq_join_build: NULL pointer");
    if (n1 > 0x7FFFFFFFull) return set_err(MQ_EINVAL, "mq_join_build: build side over 2^31 rows");
    hipStream_t st = (hipStream_t)stream;
    mq_join* j = new mq_join();
    std::memset(j, 0, sizeof(*j));
    HIPCHK(hipGetDevice(&j->device));
    j->stream = st;
    if ((rc = build_into(j, d_c1, d_p1, n1, st, s, true))) {
        jfree_all(j);
        delete j;
        return rc;
    }
    *out = j;
    return MQ_OK;
}

int mq_join_probe(mq_join* j, const int32_t* d_c2, uint64_t n2, uint64_t* h_m, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!j || !h_m || (n2 && !d_c2)) return set_err(MQ_EINVAL, "mq_join_probe: bad argument");
    if (n2 > (1ull << 31)) return set_err(MQ_EINVAL, "mq_join_probe: %llu rows (int32 positions)", (unsigned long long)n2);
    hipStream_t st = (hipStream_t)stream;
    if ((rc = juse(j, st))) return rc;
    // a queued write may still read the last probe's arrays: freed in stream order
    release_probe(j, st);
    j->pr.n2 = n2;
    j->pr.m = 0;
    j->pr.longcap = 0;
    *h_m = 0;
    if (n2 == 0 || j->n1 == 0) return MQ_OK;
    // a partitioned build and a probe side too small to pay for its own partition (its
    // passes and the window join read all n1 build words): the global table, once
    const uint64_t small = small_probe_rows(j);
    if (j->dupw && n2 < small) {  // duplicate keys, a small probe: a runs table
        if ((rc = rebuild_unpartitioned(j, st))) return rc;
        return mq_join_probe(j, d_c2, n2, h_m, stream);
    }
    if (j->part && n2 < small) {
        bool flagged = false;
        if ((rc = materialize_table(j, st, &flagged))) return rc;
        if (flagged) {
            if ((rc = rebuild_unpartitioned(j, st))) return rc;
            return mq_join_probe(j, d_c2, n2, h_m, stream);
        }
    }
    // the partitioned probes of a unique build and of duplicate keys on the partitioned
    // words: up to the window join and all but the last inverse pass; M from the window
    // joins' pair count, the rest in mq_join_write (k_pwin_gather_write)
    if (j->dupw || (j->unique == 1 && j->part)) {
        j->pr.pruns = j->pr.run2 = j->dupw;
        HIPCHK(hipMemsetAsync(j->pflag, 0, 4, st));
        HIPCHK(hipMemsetAsync(j->mtot, 0, 8, st));
        if ((rc = probe_partitioned_deferred(j, d_c2, n2, st))) return rc;
        uint32_t pf = 0;
        unsigned long long mm = 0;
        HIPCHK(hipMemcpyAsync(&pf, j->pflag, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&mm, j->mtot, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (pf) {
            // a probe key met a duplicate build key: the same partitioned words answer
            // duplicate keys (k_win_join_runs) when a payload value is free; otherwise, an
            // overfull window or a key on 15+ rows: rebuild from the inputs on the runs tables
            if (pf == 1u && !j->dupw && j->rsent_ok && dupw_allowed()) {
                if ((rc = make_dupw(j))) return rc;
            } else if ((rc = rebuild_unpartitioned(j, st))) {
                return rc;
            }
            return mq_join_probe(j, d_c2, n2, h_m, stream);
        }
        j->pr.m = mm;
        *h_m = mm;
        return MQ_OK;
    }
    const uint64_t nwords = (n2 + 63) / 64;
    // packed runs: per-word lengths. Only for the windowed runs build (rs == nullptr:
    // every run shorter than 15 rows), where a word's 64 rows sum to < 2^10; a sorted
    // runs build may hold runs of up to n1 rows, whose sums over a word would wrap the
    // u32 word counts and the write's u32 wave prefix, so it takes the per-row form
    // (u32 lengths, u64 offsets).
    const bool pruns = j->unique == 2 && j->packed && j->rs == nullptr;
    j->pr.pruns = pruns;
    j->pr.run2 = false;
    const bool words_scan = j->unique == 1 || pruns;  // per 64-row word; else per row
    j->pr.pstart = (uint32_t*)pool_alloc(n2 * 4);
    j->pr.plen = (uint32_t*)pool_alloc(j->unique == 1 ? nwords * 12 : pruns ? nwords * 4 : n2 * 4);
    j->pr.offs = (u64*)pool_alloc((words_scan ? nwords : n2) * 8);
    j->pr.scan_scratch = (u64*)pool_alloc(scan_u32_scratch_elems(words_scan ? nwords : n2) * 8);
    if (!j->pr.pstart || !j->pr.plen || !j->pr.offs || !j->pr.scan_scratch)
        return set_err(MQ_ENOMEM, "mq_join_probe: buffers for %llu rows", (unsigned long long)n2);
    // unique path: plen holds one 64-bit hit word per 64 rows, then those words'
    // popcounts; offs the words' output offsets. Otherwise both are per row.
    const uint64_t nw = (n2 + 63) / 64;
    const uint64_t nscan = words_scan ? nw : n2;
    uint32_t* const cnt = j->unique == 1 ? j->pr.plen + 2 * nw : j->pr.plen;
    if (pruns && j->win.wlog == kWinLog && j->n1 >= part_min_rows() && n2 >= small) {
        // packed runs, partitioned: the probe keys by window, each window's slice of the runs
        // table in LDS (no free payload value for run2 records, or forced by a test)
        if ((rc = probe_partitioned_runs(j, d_c2, n2, j->pr.pstart, cnt, st))) return rc;
    } else if (j->unique) {
        if ((rc = probe_table(s, j, d_c2, n2, cnt, st))) return rc;
    } else {
        hipLaunchKernelGGL(k_ht_probe, dim3(stream_grid(s, n2)), dim3(kTPB), 0, st, d_c2, n2,
                           j->words, j->start, j->len, j->mask, j->pr.pstart, j->pr.plen);
        LAUNCHCHK("k_ht_probe");
    }
    if ((rc = scan_u32_exclusive(cnt, j->pr.offs, nscan, j->pr.scan_scratch, st))) return rc;
    u64 last_off = 0;
    uint32_t last_len = 0;
    HIPCHK(hipMemcpyAsync(&last_off, j->pr.offs + (nscan - 1), 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&last_len, cnt + (nscan - 1), 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    j->pr.m = last_off + last_len;
    *h_m = j->pr.m;
    return MQ_OK;
}

int mq_join_write(mq_join* j, const int32_t* d_p2, int32_t* d_out1, int32_t* d_out2, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!j) return set_err(MQ_EINVAL, "mq_join_write: NULL handle");
    if (j->pr.m == 0) return MQ_OK;
    if (!d_out1 || (d_out2 && !d_p2)) return set_err(MQ_EINVAL, "mq_join_write: NULL pointer");
    if ((rc = juse(j, (hipStream_t)stream))) return rc;
    if (j->pr.deferred) return write_deferred(j, d_p2, d_out1, d_out2, (hipStream_t)stream);
    if (j->unique == 1) {
        const bool v4 = ((reinterpret_cast<uintptr_t>(j->pr.pstart) | reinterpret_cast<uintptr_t>(d_p2)) & 15u) == 0;
        if (v4)
            hipLaunchKernelGGL(k_join_write_hits4, dim3(stream_grid(s, (j->pr.n2 + 3) / 4)), dim3(kTPB), 0,
                               (hipStream_t)stream, reinterpret_cast<const u64*>(j->pr.plen), j->pr.offs, j->pr.pstart, d_p2,
                               j->pr.n2, d_out1, d_out2);
        else
            hipLaunchKernelGGL(k_join_write_hits, dim3(stream_grid(s, j->pr.n2)), dim3(kTPB), 0, (hipStream_t)stream,
                               reinterpret_cast<const u64*>(j->pr.plen), j->pr.offs, j->pr.pstart, d_p2, j->pr.n2, d_out1, d_out2);
        LAUNCHCHK("k_join_write_hits");
        return MQ_OK;
    }
    if (j->pr.pruns && j->pr.run2) {
        hipLaunchKernelGGL(k_join_write_runs16<8>, dim3(stream_grid(s, ((j->pr.n2 + 63) / 64) * 64 / 8)), dim3(kTPB), 0,
                           (hipStream_t)stream, j->pr.pstart, j->pr.n2, j->pr.offs, d_p2, j->pr.p01, j->bpos, d_out1, d_out2);
        LAUNCHCHK("k_join_write_runs16");
        return MQ_OK;
    }
    if (j->pr.pruns) {
        hipLaunchKernelGGL(k_join_write_runs_mlp<8>, dim3(stream_grid(s, ((j->pr.n2 + 63) / 64) * 64 / 8)), dim3(kTPB), 0,
                           (hipStream_t)stream, j->pr.pstart, j->pr.n2, j->rs, j->pr.offs, d_p2, j->bpos, d_out1, d_out2);
        LAUNCHCHK("k_join_write_runs");
        return MQ_OK;
    }
    // the long-run list: at most m / kLongRun chunks (+ one per run for the rounding)
    const uint64_t qcap = j->pr.m / kLongRun + j->pr.m / kLongChunk + 2;
    if (qcap > 0xFFFFFFF0ull) return set_err(MQ_EINVAL, "mq_join_write: %llu pairs", (unsigned long long)j->pr.m);
    pool_free_on(j->pr.longq, (hipStream_t)stream);
    if (!(j->pr.longq = (u64*)pool_alloc(qcap * 8 + 16))) return set_err(MQ_ENOMEM, "mq_join_write: long-run list");
    j->pr.longcap = qcap;
    uint32_t* const nlong = reinterpret_cast<uint32_t*>(j->pr.longq + qcap);
    HIPCHK(hipMemsetAsync(nlong, 0, 4, (hipStream_t)stream));
    hipLaunchKernelGGL(k_join_write, dim3(stream_grid(s, j->pr.n2)), dim3(kTPB), 0, (hipStream_t)stream,
                       j->pr.pstart, j->pr.plen, j->pr.offs, d_p2,
                       j->bpos, j->pr.n2, d_out1, d_out2, j->pr.longq, nlong);
    LAUNCHCHK("k_join_write");
    hipLaunchKernelGGL(k_join_write_long, dim3(s->cus * 8), dim3(kTPB), 0, (hipStream_t)stream, j->pr.pstart, j->pr.plen,
                       j->pr.offs, d_p2, j->bpos, j->pr.longq, nlong, d_out1, d_out2);
    LAUNCHCHK("k_join_write_long");
    return MQ_OK;
}

int mq_join_counts(mq_join* j, uint32_t* d_cnt, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!j || (j->pr.n2 && !d_cnt)) return set_err(MQ_EINVAL, "mq_join_counts: bad argument");
    if (j->pr.n2 == 0) return MQ_OK;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = juse(j, st))) return rc;
    if (j->n1 == 0) {  // the probe ran nothing: no row matched
        HIPCHK(hipMemsetAsync(d_cnt, 0, j->pr.n2 * 4, st));
        return MQ_OK;
    }
    if (j->pr.deferred && (rc = finish_classic(j, st))) return rc;
    const u64* hits = j->unique == 1 ? reinterpret_cast<const u64*>(j->pr.plen) : nullptr;
    const uint32_t* pk = (!hits && j->pr.pruns) ? j->pr.pstart : nullptr;
    const uint32_t* plen = (!hits && !j->pr.pruns) ? j->pr.plen : nullptr;
    hipLaunchKernelGGL(k_join_counts, dim3(stream_grid(s, j->pr.n2)), dim3(kTPB), 0, st, hits, pk, plen, j->pr.n2, d_cnt);
    LAUNCHCHK("k_join_counts");
    return MQ_OK;
}

int mq_join_state(const mq_join* j, uint32_t* out) {
    if (!j || !out) return set_err(MQ_EINVAL, "mq_join_state: NULL pointer");
    const mqj::ProbeState& p = j->pr;
    out[0] = (uint32_t)j->unique;
    out[1] = (j->part ? MQ_JOIN_STATE_PART : 0u) | (j->dupw ? MQ_JOIN_STATE_DUPW : 0u) |
             (j->packed ? MQ_JOIN_STATE_PACKED : 0u) | (j->rs ? MQ_JOIN_STATE_RS : 0u) |
             (p.pruns ? MQ_JOIN_STATE_PRUNS : 0u) | (p.run2 ? MQ_JOIN_STATE_RUN2 : 0u) |
             (p.deferred ? MQ_JOIN_STATE_DEFERRED : 0u) | (p.longcap ? MQ_JOIN_STATE_ROW_WRITE : 0u);
    out[2] = 0;
    if (p.longcap) {  // the entry count k_join_write left behind the list
        HIPCHK(hipStreamSynchronize(j->stream));
        HIPCHK(hipMemcpy(&out[2], p.longq + p.longcap, 4, hipMemcpyDeviceToHost));
    }
    return MQ_OK;
}

int mq_random_read(const uint64_t* d_table, int slots_log2, uint64_t n_reads, void* d_ws, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (!d_table || !d_ws) return set_err(MQ_EINVAL, "mq_random_read: NULL pointer");
    if (slots_log2 < 0 || slots_log2 > 40) return set_err(MQ_EINVAL, "mq_random_read: slots_log2 %d", slots_log2);
    if (n_reads == 0) return MQ_OK;
    hipLaunchKernelGGL(k_random_read, dim3(stream_grid(s, (n_reads + kProbeILP - 1) / kProbeILP)), dim3(kTPB), 0,
                       (hipStream_t)stream, reinterpret_cast<const u64*>(d_table), (1ull << slots_log2) - 1,
                       n_reads, static_cast<u64*>(d_ws));
    LAUNCHCHK("k_random_read");
    return MQ_OK;
}

int mq_join_free(mq_join* j) {
    if (!j) return MQ_OK;
    // queued probe / write kernels may still use the buffers: freed in j->stream's order
    release_probe(j, j->stream);
    pool_free_on(j->pr.longq, j->stream);
    jfree_all(j);
    delete j;
    return MQ_OK;
}

int mq_hash_join(const int32_t* d_c1, const int32_t* d_p1, uint64_t n1, const int32_t* d_c2,
                 const int32_t* d_p2, uint64_t n2, int32_t* d_out1, int32_t* d_out2,
                 uint64_t cap, uint64_t* h_m, void* stream) {
    if (!h_m) return set_err(MQ_EINVAL, "mq_hash_join: NULL h_m");
    mq_join* j = nullptr;
    int rc = mq_join_build(d_c1, d_p1, n1, &j, stream);
    if (rc) return rc;
    if ((rc = mq_join_probe(j, d_c2, n2, h_m, stream))) {
        mq_join_free(j);
        return rc;
    }
    if (*h_m > cap || !d_out1 || !d_out2) {
        mq_join_free(j);
        return *h_m == 0 ? MQ_OK : MQ_ECAP;
    }
    const bool fused = j->pr.deferred;
    rc = mq_join_write(j, d_p2, d_out1, d_out2, stream);
    if (!rc) rc = mq_stream_sync(stream);
    if (!rc && fused) {  // the fused write's look-back gave up (never expected): fail loudly
        uint32_t e = 0;
        if (hipMemcpy(&e, j->pflag + 1, 4, hipMemcpyDeviceToHost) != hipSuccess || e)
            rc = set_err(MQ_EHIP, "mq_hash_join: the fused write's look-back failed");
    }
    mq_join_free(j);
    return rc;
}

}  // extern "C"

