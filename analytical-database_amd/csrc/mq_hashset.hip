// mq_hashset.hip — hashset.c's insert loop (src/hashset.c:25-32) as a bulk build on gfx950.
//
// mq_hashset_insert leaves in the int32 table exactly the slots that
//   for i in 0..n-1: insert_hashset(set, keys[i])
// leaves, whatever order the blocks run in.
//
// The sequential layout is the unique one in which every stored key k at slot s has,
// in each slot of the cyclic range [home(k), s), a key inserted before it. So a key's
// priority is its insertion order: the resident keys first (they never move), then the
// new keys by first occurrence. The build is a priority-ordered linear probe over a
// 64-bit working copy of the table, one word (priority << 32 | key) per slot:
//   k_hs_expand : table -> words; a resident key has priority 0xFFFFFFFF, an empty
//                 slot is word 0 (the lowest).
//   k_hs_first  : the first occurrence of every distinct nonzero key, in a scratch
//                 open-addressing table (a power of two of >= 2n slots, mixing hash):
//                 a compare-and-swap claims a slot for a key, an atomicMin keeps the
//                 lowest index. Two copies of one key would otherwise pass each other
//                 in the probe (the later one evicted past a slot the earlier one then
//                 settles in) and both stay.
//   k_hs_insert : one lane per scratch slot. The lane carries a word from its key's
//                 home slot: a slot of lower priority takes the word by a 64-bit
//                 compare-and-swap and the lane carries the evicted word on from the
//                 next slot; a slot of higher priority is stepped over; the same key (a
//                 resident copy) ends the walk, as does an empty slot taken. A word
//                 whose displacement from its own home reaches `size` is dropped: it
//                 has seen `size` slots of higher priority, the table is full without it.
//   k_hs_pack   : words -> table, and the number of nonzero slots.
// No lane waits for another: every successful compare-and-swap strictly raises its
// slot's word, every failed one has seen the slot raised by someone else, so the walks
// end. Stream order between the kernels gives visibility; the atomics are relaxed,
// device scope.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mq_common.h"
#include "mq_device.h"

namespace {

using namespace mqi;

constexpr int kTPB = 256;
constexpr unsigned long long kEmptyFirst = ~0ull;  // scratch: no key yet
constexpr uint32_t kResident = 0xFFFFFFFFu;        // priority of a key already in the table

using u64 = unsigned long long;

__device__ __forceinline__ u64 ld(const u64* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t hs_home(int32_t key, int32_t size) {
    int32_t idx = key % size;  // hash() of multimap.c:60-63
    return (uint32_t)(idx < 0 ? idx + size : idx);
}

// murmur3's 32-bit finaliser: spreads keys that share key % size over the scratch
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

__global__ __launch_bounds__(kTPB) void k_hs_expand(const int32_t* __restrict__ table, uint32_t size,
                                                    u64* __restrict__ words) {
    const uint32_t stride = gridDim.x * kTPB;
    for (uint64_t s = (uint64_t)blockIdx.x * kTPB + threadIdx.x; s < size; s += stride) {
        const uint32_t v = (uint32_t)table[s];
        words[s] = v ? ((u64)kResident << 32) | v : 0ull;
    }
}

// first[slot] = key << 32 | lowest index of key, for every distinct nonzero key
__global__ __launch_bounds__(kTPB) void k_hs_first(const int32_t* __restrict__ keys, uint64_t n,
                                                   u64* __restrict__ first, uint64_t mask) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x; i < n; i += stride) {
        const uint32_t key = (uint32_t)keys[i];
        if (key == 0) continue;  // 0 marks an empty slot: never stored
        const u64 mine = ((u64)key << 32) | i;  // i < 2^32 - 1, so never kEmptyFirst
        uint64_t slot = mix32(key) & mask;
        for (;;) {  // the scratch is at most half full: an empty slot is always ahead
            u64 cur = ld(first + slot);
            if (cur == kEmptyFirst) {
                cur = atomicCAS(first + slot, kEmptyFirst, mine);
                if (cur == kEmptyFirst) break;
            }
            if ((uint32_t)(cur >> 32) == key) {  // the slot is this key's for good
                if (cur > mine) atomicMin(first + slot, mine);
                break;
            }
            slot = (slot + 1) & mask;
        }
    }
}

__global__ __launch_bounds__(kTPB) void k_hs_insert(const u64* __restrict__ first, uint64_t slots,
                                                    u64* __restrict__ words, int32_t size) {
    const uint64_t stride = (uint64_t)gridDim.x * kTPB;
    for (uint64_t f = (uint64_t)blockIdx.x * kTPB + threadIdx.x; f < slots; f += stride) {
        const u64 e = first[f];
        if (e == kEmptyFirst) continue;
        // earlier first occurrence = higher priority; below every resident key, above empty
        u64 w = ((u64)(kResident - 1u - (uint32_t)e) << 32) | (e >> 32);
        uint32_t pos = hs_home((int32_t)(uint32_t)w, size);
        uint32_t disp = 0;  // slots between the carried word's home and pos
        u64 cur = ld(words + pos);
        for (;;) {
            if (cur < w) {
                const u64 old = atomicCAS(words + pos, cur, w);
                if (old != cur) {  // the slot was raised meanwhile: look at it again
                    cur = old;
                    continue;
                }
                if (old == 0) break;  // took an empty slot
                w = old;              // carry the evicted word on
                const uint32_t h = hs_home((int32_t)(uint32_t)w, size);
                disp = pos >= h ? pos - h : pos + (uint32_t)size - h;
            } else if ((uint32_t)cur == (uint32_t)w) {
                break;  // the key is resident
            }
            if (++disp >= (uint32_t)size) break;  // one lap without a slot: dropped
            pos = pos + 1 == (uint32_t)size ? 0 : pos + 1;
            cur = ld(words + pos);
        }
    }
}

// words == nullptr: count the table as it is (n == 0)
__global__ __launch_bounds__(kTPB) void k_hs_pack(const u64* __restrict__ words, int32_t* __restrict__ table,
                                                  uint32_t size, u64* __restrict__ stored) {
    __shared__ uint32_t s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const uint32_t stride = gridDim.x * kTPB;
    uint32_t mine = 0;
    for (uint64_t s = (uint64_t)blockIdx.x * kTPB + threadIdx.x; s < size; s += stride) {
        int32_t v;
        if (words) {
            v = (int32_t)(uint32_t)words[s];
            table[s] = v;
        } else {
            v = table[s];
        }
        mine += v != 0;
    }
    if (!stored) return;
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(stored, (u64)s_cnt);
}

uint64_t first_slots(uint64_t n) {  // a power of two of at least 2n slots
    uint64_t s = 2;
    while (s < 2 * n) s <<= 1;
    return s;
}

}  // namespace

extern "C" {

size_t mq_hashset_insert_workspace_bytes(uint64_t size, uint64_t n) {
    return (size_t)size * 8 + (n ? (size_t)first_slots(n) * 8 : 0) + 16;
}

int mq_hashset_insert(int32_t* d_table, int32_t size, const int32_t* d_keys, uint64_t n, uint64_t* d_stored,
                      void* d_ws, size_t ws_bytes, void* stream) {
    DevState* s;
    int rc = ensure_ready(&s);
    if (rc) return rc;
    if (size <= 0) return set_err(MQ_EINVAL, "mq_hashset_insert: size %d", size);
    if (!d_table || (n && !d_keys)) return set_err(MQ_EINVAL, "mq_hashset_insert: NULL pointer");
    if (n >= 0xFFFFFFFFull) return set_err(MQ_EINVAL, "mq_hashset_insert: n beyond 32-bit ranks");
    if (n && (!d_ws || ws_bytes < mq_hashset_insert_workspace_bytes((uint64_t)size, n)))
        return set_err(MQ_EINVAL, "mq_hashset_insert: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    u64* stored = reinterpret_cast<u64*>(d_stored);
    if (stored) HIPCHK(hipMemsetAsync(stored, 0, sizeof(u64), st));
    if (n == 0) {
        if (stored) {
            hipLaunchKernelGGL(k_hs_pack, dim3(stream_grid(s, (uint64_t)size)), dim3(kTPB), 0, st,
                               static_cast<const u64*>(nullptr), d_table, (uint32_t)size, stored);
            LAUNCHCHK("k_hs_pack");
        }
        return MQ_OK;
    }
    u64* words = static_cast<u64*>(d_ws);
    u64* first = words + size;
    const uint64_t slots = first_slots(n);
    HIPCHK(hipMemsetAsync(first, 0xFF, slots * 8, st));
    hipLaunchKernelGGL(k_hs_expand, dim3(stream_grid(s, (uint64_t)size)), dim3(kTPB), 0, st, d_table,
                       (uint32_t)size, words);
    LAUNCHCHK("k_hs_expand");
    hipLaunchKernelGGL(k_hs_first, dim3(stream_grid(s, n)), dim3(kTPB), 0, st, d_keys, n, first, slots - 1);
    LAUNCHCHK("k_hs_first");
    hipLaunchKernelGGL(k_hs_insert, dim3(stream_grid(s, slots)), dim3(kTPB), 0, st, first, slots, words, size);
    LAUNCHCHK("k_hs_insert");
    hipLaunchKernelGGL(k_hs_pack, dim3(stream_grid(s, (uint64_t)size)), dim3(kTPB), 0, st, words, d_table,
                       (uint32_t)size, stored);
    LAUNCHCHK("k_hs_pack");
    return MQ_OK;
}

}  // extern "C"
