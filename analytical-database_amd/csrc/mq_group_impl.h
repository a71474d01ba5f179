// mq_group_impl.h — internal (not exported) entry points of mq_group.hip that mq_measures.hip
// and mq_distinct.hip share: the tuple code of a row's key columns, the key space of a tuple's
// bounds, and the launches of the sort path's kernels that serve any column of codes (the joined
// rows' codes through their positions, the count of rows out of bounds, the run heads of the
// sorted codes, the decode of a group's code into its keys). Each launch queues on `st` and leaves
// hipGetLastError() to the caller, unless it returns a code itself.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mq_where_common.h"

namespace mqi {

// The tuple code of up to MQ_GROUP_MAX_KEYS key columns as kernel arguments: a row's code is the
// sum of (K_j - lo_j) * stride_j, the last column running fastest.
struct ByArgs {
    const int* keys[MQ_GROUP_MAX_KEYS];
    uint32_t lo[MQ_GROUP_MAX_KEYS];
    uint32_t rm1[MQ_GROUP_MAX_KEYS];     // range - 1: a range of 2^32 has no u32
    uint32_t stride[MQ_GROUP_MAX_KEYS];  // mod 2^32: a stride of 2^32 (held as 0) only meets K_j - lo_j = 0
};

// The code of one row's tuple; *in: every component lies within its own column's bounds. A
// check of the sum would not do: (3, 12) under ranges (10, 10) sums to 42, inside the table.
template <int NK>
__device__ __forceinline__ uint32_t row_code(const ByArgs& a, const int (&k)[NK], bool* in) {
    uint32_t c = 0;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < NK; j++) {
        const uint32_t d = (uint32_t)k[j] - a.lo[j];  // a key below lo wraps past the range
        ok = ok && d <= a.rm1[j];
        c += d * a.stride[j];
    }
    *in = ok;
    return c;
}

__device__ __forceinline__ int elem(const int4& q, int e) { return e == 0 ? q.x : e == 1 ? q.y : e == 2 ? q.z : q.w; }

// The codes of a lane's four rows of one tile; bit e of *in: row e is within the bounds.
template <int NK>
__device__ __forceinline__ uint4 tile_codes(const ByArgs& a, const int4 (&k)[NK], uint32_t* in) {
    uint32_t c[4], m = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        int r[NK];
#pragma unroll
        for (int j = 0; j < NK; j++) r[j] = elem(k[j], e);
        bool ok;
        c[e] = row_code<NK>(a, r, &ok);
        m |= ok ? 1u << e : 0u;
    }
    *in = m;
    return make_uint4(c[0], c[1], c[2], c[3]);
}

// *space = prod(hi_j - lo_j + 1) over the nkeys {lo, hi} pairs of b, saturated at 2^63; false: a lo > hi.
bool group_key_space(const int32_t* b, int nkeys, uint64_t* space);
// k_group_star_pack_pos<a.nterms> on `grid` blocks: packed[i] = code(row pos[i]) + add for i < k;
// bad holds grid * kWaves counts of rows with a component out of bounds.
void group_launch_star_pack_pos(const StarArgs& a, uint32_t grid, const int32_t* pos, uint32_t k, uint32_t n, uint32_t add,
                                int32_t* packed, uint32_t* bad, hipStream_t st);
// k_group_by_where_bounds and its fold over nkeys (1..4) key columns: *rows = the rows that match w,
// bounds[2j], bounds[2j + 1] = column j's min and max over them (INT_MAX, INT_MIN without one).
// Synchronises; returns MQ_OK or the error it recorded under `who`.
int group_where_key_bounds(const DevState* s, const WhereArgs& w, bool vec, const int32_t* const* d_keys, int nkeys, uint64_t n,
                           uint64_t* rows, int32_t* bounds, hipStream_t st, const char* who);
// k_group_by_pack (pos == NULL: packed[i] = code(row i) ^ 0x80000000, i < n) or k_group_by_pack_pos
// (packed[i] = code(row pos[i]) ^ 0x80000000, i < k) over nkeys (1..4) key columns; *bad (pool_alloc'd,
// the caller frees it) holds *nbad counts of rows with a component out of bounds. Returns a code.
int group_launch_pack(const DevState* s, const ByArgs& a, int nkeys, uint64_t n, const int32_t* pos, uint64_t k, int32_t* packed,
                      uint32_t** bad, uint32_t* nbad, hipStream_t st);
// k_group_by_bad: *total = the sum of nbad counts.
void group_launch_bad_total(const uint32_t* bad, uint32_t nbad, unsigned long long* total, hipStream_t st);
// k_group_heads over mq_group_sort_geometry(n)'s grid: ccnt[b] = run heads in chunk b, added up onto *groups.
void group_launch_heads(const int32_t* sorted, uint32_t n, uint64_t chunk, uint32_t blocks, uint32_t* ccnt,
                        unsigned long long* groups, hipStream_t st);
// k_group_by_unpack: codes[i] ^ flip decoded into keys_out[j][i] (NULL entries skipped), j < nkeys.
void group_launch_unpack(const int32_t* codes, uint64_t groups, const int32_t* klo, const uint32_t* krm1, const uint32_t* kstride,
                         int nkeys, uint32_t flip, int32_t* const* keys_out, uint32_t grid, hipStream_t st);

// What mq_topk64.hip lends mq_group_top, on `grid` blocks of a grid-stride loop each:
// k_topk64_widen: out[i] = in[i] sign-extended, i < n.
void topk64_launch_widen(const int32_t* in, uint64_t n, int64_t* out, uint32_t grid, hipStream_t st);
// k_topk64_take: out[i] = col[idx[i]], i < m.
void topk64_launch_take32(const int32_t* col, const uint32_t* idx, uint64_t m, int32_t* out, uint32_t grid, hipStream_t st);
void topk64_launch_take64(const int64_t* col, const uint32_t* idx, uint64_t m, int64_t* out, uint32_t grid, hipStream_t st);

}  // namespace mqi
