// mq_group_impl.h — internal (not exported) entry points of mq_group.hip that mq_measures.hip
// shares: the key space of a tuple's bounds, and the launches of the sort path's kernels that
// serve any column of codes (the joined rows' codes through their positions, the count of rows
// out of bounds, the run heads of the sorted codes, the decode of a group's code into its keys).
// Each launch queues on `st` and leaves hipGetLastError() to the caller.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mq_where_common.h"

namespace mqi {

// *space = prod(hi_j - lo_j + 1) over the nkeys {lo, hi} pairs of b, saturated at 2^63; false: a lo > hi.
bool group_key_space(const int32_t* b, int nkeys, uint64_t* space);
// k_group_star_pack_pos<a.nterms> on `grid` blocks: packed[i] = code(row pos[i]) + add for i < k;
// bad holds grid * kWaves counts of rows with a component out of bounds.
void group_launch_star_pack_pos(const StarArgs& a, uint32_t grid, const int32_t* pos, uint32_t k, uint32_t n, uint32_t add,
                                int32_t* packed, uint32_t* bad, hipStream_t st);
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
