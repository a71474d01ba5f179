// mq_join_impl.h — internal to the hash join: the handle, the table's device helpers and
// the host functions through which its two halves talk. mq_join.hip holds the global-table,
// runs and write kernels, the build policy and the C API; mq_join_part.hip the window
// partition and everything that works window by window in LDS. Neither launches the
// other's kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "mq_common.h"
#include "mq_device.h"
#include "mq_radix.h"

// (hidden: libmq.so exports none of this)
namespace mqj __attribute__((visibility("hidden"))) {

using namespace mqi;

// Test and A/B knobs, read from the environment on every call (tests flip them between
// calls in one process):
//   MQ_JOIN_PART=0      no partitioned build: the global table always
//   MQ_JOIN_PART_MIN=n  the partitioned build from n build rows (default 2^20)
//   MQ_JOIN_PART_DIV=d  a probe of fewer than n1 / d rows takes the global table (default 16)
//   MQ_JOIN_SAMPLE=0    no sampled duplicate check: the unique build is attempted first
//   MQ_JOIN_NARROW=0    the window join's results as u64 words, not u32 payloads; a windowed
//                       runs table then also carries no short runs' positions (no run2)
//   MQ_JOIN_RUN2=0      duplicate keys on a runs table, not on the partitioned words
//   MQ_JOIN_WINRUNS=0   duplicate keys on the sorted-runs build, not the windowed one
//   MQ_JOIN_RUNS=0      duplicate keys on the global-CAS table of run heads
inline bool knob_off(const char* name) {
    const char* e = getenv(name);
    return e && e[0] == '0';
}
inline uint64_t knob_u64(const char* name, uint64_t dflt) {
    const char* e = getenv(name);
    return e ? strtoull(e, nullptr, 10) : dflt;
}

// ---------------------------------------------------------------------------
// hash table: 64-bit slot words {key (low 32), occupied (bit 32)}, linear probing
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t hash32(uint32_t k) {  // murmur3 finaliser
    k ^= k >> 16;
    k *= 0x85EBCA6Bu;
    k ^= k >> 13;
    k *= 0xC2B2AE35u;
    k ^= k >> 16;
    return k;
}

__device__ __forceinline__ u64 pack_key(int key) { return (u64)(uint32_t)key | (1ull << 32); }

// Unique-key table: one 64-bit word per slot, {key (low 32), build payload = the
// build position p1[row] (high 32)}; all-ones = empty. One CAS per build row, and a
// probe hit yields out1's value directly (no gather from p1). A build row whose
// word equals the empty marker (key = p1 = -1) sends the build to the general path.
constexpr u64 kEmpty = ~0ull;
__device__ __forceinline__ u64 pack_pair(int key, int payload) {
    return (u64)(uint32_t)key | ((u64)(uint32_t)payload << 32);
}

// Windowed open addressing: the table is cut into windows of W = min(8192, slots)
// slots and linear probing wraps inside the key's home window, so a window can be
// built in LDS (64 KB) and written out with one coalesced sweep.
constexpr int kWinLog = 13;
constexpr int kWinTPB = 1024;

struct Win {
    uint64_t mask;   // slots - 1
    uint64_t wmask;  // W - 1
    int wlog;        // log2 W
};

__device__ __forceinline__ uint64_t win_next(uint64_t h, const Win& t) {
    return (h & ~t.wmask) | ((h + 1) & t.wmask);
}
__device__ __forceinline__ uint32_t win_id(uint32_t key, const Win& t) {
    return (uint32_t)((hash32(key) & t.mask) >> t.wlog);
}

// Unique-key tables start a key's linear probe at the first slot of its aligned
// 4-slot bucket (32 B), not at its own slot: a probe then reads the whole bucket
// with two 16-byte loads and rarely needs a second, dependent read (with the probe
// starting at the hashed slot itself, about every other probe at load 1/2 went on
// to the next slot after its first read returned).
constexpr uint32_t kBucket = 4;
__device__ __forceinline__ uint64_t ht_home(uint32_t key, uint64_t mask) {
    return hash32(key) & mask & ~(uint64_t)(kBucket - 1);
}
// a full bucket's overflow mark (windowed builds, k_win_build): slot order
__device__ __forceinline__ bool bucket_ovf(u64 s0, u64 s1) { return (uint32_t)s0 > (uint32_t)s1; }

// Unique-path build.
//  * below kWindowBuildRows: one global CAS per build row (the table is small);
//  * above: stable LSD radix partition of the (key, payload) words by window id,
//    then one block per window builds it in LDS and stores it whole (no global
//    atomics; every window is written, so the table needs no memset).
// (A partition by table window feeding the global-CAS insert measured 20.3 vs
// 21.0 ms at 2^28 rows plus the partition pass: device-scope CAS costs the same
// wherever the line lives, so the atomics themselves have to go.)
constexpr uint64_t kWindowBuildRows = 1ull << 16;

// What the last probe left for mq_join_write / mq_join_counts (pool blocks, released
// together: release_probe).
struct ProbeState {
    uint64_t n2, m;
    bool pruns;            // the last probe took the per-64-row-word form (packed runs of < 15 rows)
    bool run2;             // the last probe left short runs' positions in p01 (k_join_write_runs16)
    u64* p01;              // run2: per probe row, a short run's build positions
    uint32_t* pstart;
    uint32_t* plen;
    u64* offs;
    u64* scan_scratch;
    u64* longq;            // per-row write: chunks of the long runs (k_join_write_long)
    uint64_t longcap;      // ... its capacity (the entry count follows it); 0: no per-row write
                           // since the last probe (mq_join_state)
    // deferred (round 6): the partitioned probe stopped before its last inverse pass, which
    // mq_join_write runs fused with the pair write (dmode: 0 unique u32 results, 1 unique
    // u64, 2 run2 records); dperm = pass 0's places of the probe rows (pool, owned),
    // dhs0 = pass 0's tile offsets, dres = the results in pass-0 order (pool, owned)
    bool deferred;
    int dmode;
    uint16_t* dperm;
    u64* dhs0;
    void* dres;
};

}  // namespace mqj

// ===========================================================================
// handle
// ===========================================================================
struct mq_join {
    int device;
    int unique;            // 1: windowed {key, payload} table (words only); 0: words/start/len;
                           // 2: windowed table of distinct keys -> run index, runs in rs
    const uint32_t* rs;    // unique == 2: first sorted row of each run, + n1
    bool marks;            // the unique table's full buckets carry overflow marks (k_win_build)
    bool packed;           // unique == 2: payloads carry start << 4 | length (k_run_payload)
    uint64_t n1, mask;
    mqj::Win win;          // unique table geometry
    mqi::u64* words;
    uint32_t* start;
    uint32_t* len;
    const int* bpos;       // build positions in run order (p1 itself, or sorted copy)
    void* owned[16];       // device allocations owned by the handle
    int nowned;
    mqj::ProbeState pr;
    hipStream_t stream;    // the stream of the handle's last queued work (juse)
    // partitioned unique build (round 5): no global table; the build's words partitioned
    // by window (pwords) and each window's first word (pwstart, nwin + 1 entries); the
    // probe partitions its keys the same way (passes LSD passes) and joins window by
    // window in LDS (probe_partitioned). words == nullptr until a probe asks for the table.
    bool part;
    const int32_t* c1;     // the build inputs (valid until mq_join_free): a partitioned build
    const int32_t* p1;     // that meets a duplicate key or an overfull window is rebuilt
    uint32_t* pflag;       // the window join's flag (a duplicate met, a window overfull)
    bool narrow;           // the window join's results as u32 payloads, `sentinel` = a miss
    bool dupw;             // a partitioned build whose probe answers duplicate keys window by
                           // window (k_win_join_runs: run2 records, long runs into bpos)
    unsigned long long* mtot;  // the window joins' pair count (device)
    bool rsent_ok;         // windowed runs: `sentinel` is outside the payloads (the partitioned
                           // runs probe then carries short runs' positions, run2)
    uint32_t sentinel;     // (a value outside the build payloads' range)
    mqi::u64* pwords;
    uint32_t* pwstart;
    uint32_t nwin;
    int passes;
    uint64_t slots;
};

namespace mqj __attribute__((visibility("hidden"))) {

// What a deferred probe kept for its last inverse pass, given back (stream-ordered).
inline void release_deferred(mq_join* j, hipStream_t st) {
    ProbeState& p = j->pr;
    pool_free_on(p.dhs0, st);
    pool_free_on(p.dres, st);
    pool_free_on(p.dperm, st);
    p.dhs0 = nullptr;
    p.dres = nullptr;
    p.dperm = nullptr;
    p.deferred = false;
}

// The last probe's arrays given back in stream order (a queued write may still read them).
// longq is the write's, not the probe's: mq_join_write and mq_join_free free it.
inline void release_probe(mq_join* j, hipStream_t st) {
    ProbeState& p = j->pr;
    pool_free_on(p.p01, st);
    pool_free_on(p.pstart, st);
    pool_free_on(p.plen, st);
    pool_free_on(p.offs, st);
    pool_free_on(p.scan_scratch, st);
    p.p01 = nullptr;
    p.pstart = p.plen = nullptr;
    p.offs = p.scan_scratch = nullptr;
    release_deferred(j, st);
}

// ---- mq_join.hip ----
// The handle's own allocations (freed with it; jdrop gives one back early, stream-ordered).
int jown(mq_join* j, void* p);
int jalloc(mq_join* j, void** p, size_t bytes);
void jdrop(mq_join* j, void* p);
// cnt[w] = popcount(hits[w]) for the nw hit words of a unique probe.
int hits_count(const DevState* s, const u64* hits, uint64_t nw, uint32_t* cnt, hipStream_t st);
// The payloads' range folded from the 64 min / 64 max slots the partition's first scatter
// left (sl, read back by the caller): j->sentinel = a value outside it, the marker of a
// miss, and j->rsent_ok = one exists. MQ_JOIN_NARROW=0 turns off j->narrow (the window
// join's u32 results), or with narrow_gates_rsent (a windowed runs table) rsent_ok itself.
void fold_payload_range(mq_join* j, const int (&sl)[128], bool narrow_gates_rsent);

// ---- mq_join_part.hip ----
// The global unique table of n >= kWindowBuildRows rows, built window by window into
// j->words (*general: a duplicate key, the empty word or an overfull window). Synchronises.
int win_build_table(mq_join* j, const int* c1, const int* p1, uint64_t n, uint64_t slots, uint32_t* general,
                    hipStream_t st);
// The partitioned build: the window partition alone, kept by the handle (pwords, pwstart,
// nwin, passes; checked by the probe), the payloads' range into pmm.
int win_keep_partition(mq_join* j, const int* c1, const int* p1, uint64_t n, uint64_t slots, int* pmm,
                       hipStream_t st);
int build_window_runs(mq_join* j, const int* c1, const int* p1, uint64_t n, uint64_t slots, uint32_t* general,
                      hipStream_t st, int* pmm);
// The partitioned probe of a partitioned build (unique keys, or dupw) up to its last
// inverse pass, which is left to write_deferred (or finish_classic); sets j->pr.dmode.
int probe_partitioned_deferred(mq_join* j, const int32_t* d_c2, uint64_t n2, hipStream_t st);
int probe_partitioned_runs(mq_join* j, const int32_t* d_c2, uint64_t n2, uint32_t* pstart, uint32_t* wcnt,
                           hipStream_t st);
int finish_classic(mq_join* j, hipStream_t st);
int write_deferred(mq_join* j, const int32_t* d_p2, int32_t* d_out1, int32_t* d_out2, hipStream_t st);
int materialize_table(mq_join* j, hipStream_t st, bool* flagged);

}  // namespace mqj

