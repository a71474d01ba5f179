/*
 * mq_device.h — device-level C-ABI of libmq (MI355X / gfx950 column-scan executor).
 *
 * Plain pointers, sizes and a `void* stream` (a hipStream_t; NULL = the HIP null
 * stream; mq_default_stream() returns the library's own non-blocking stream). Every column / position pointer below is a DEVICE
 * pointer into HBM. All functions return 0 (MQ_OK) on success or a negative
 * MQ_E* code; mq_last_error() returns a message for the calling thread's last
 * failure. Nothing here falls back to the CPU: without a usable gfx950 device
 * every entry point returns MQ_ENODEV.
 *
 * Predicates are the reference's half-open range select: a row v matches when
 * (!has_low || v >= low) && (!has_high || v < high)  (src/query.c:97-127).
 *
 * The reference-facing drop-in (select_column, fetch_column, sum, ...) is in
 * mq_query.h; it is implemented in C on top of these entry points.
 *
 * Threads: any number of host threads may be inside these entry points at once, each
 * on streams, buffers and workspaces of its own (tests/test_gpu_threads.py).
 * Per thread: mq_last_error()'s message (the empty string until a call of the thread
 *   fails); the delete plan and the insert plan (an apply step on a thread that made no
 *   plan on that workspace is MQ_EINVAL); the state mq_shared_select_count leaves for
 *   mq_shared_select_write; the pinned staging of the staged copies, the segmented
 *   download and shared_select, freed by mq_thread_release(), which is a thread's last
 *   libmq call.
 * Shared, behind locks: the mq_pool_* allocator that every operator's scratch comes
 *   from; the per-kernel occupancy cache; the arrival counters of the folded one-launch
 *   forms (mq_select_agg, mq_select_sum, mq_select_fetch_agg, mq_reduce), one block per
 *   device and stream, per thread as well for the per-thread default stream.
 * May be shared between threads: a key set and a key map, once built (immutable, probed on
 *   any stream); an mq_mgroup (mq_group_measures_write from several threads at once, into
 *   different outputs: the write kernels only read the handle's buffers. Each write also
 *   stores its stream in the handle, unsynchronised, and mq_group_measures_free frees in the
 *   order of whichever stream was stored last: after concurrent writes, free only once
 *   every write has completed, or queue one last write from the freeing thread on a live
 *   stream first); any handle that one thread plans or builds and another, after
 *   the first's work on it has completed, writes and frees. mq_group and mq_gdistinct
 *   handles are written by one thread at a time.
 * Not for concurrent use: mq_test_set_cu_limit and mq_release_all (no other thread
 *   inside libmq), and the whole of mq_query.h, whose tables have no lock.
 */
#ifndef MQ_DEVICE_H
#define MQ_DEVICE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    MQ_OK = 0,
    MQ_ENODEV = -1,   /* no gfx950 device / HIP runtime unusable */
    MQ_EINVAL = -2,   /* bad argument (NULL, misaligned, size out of range) */
    MQ_EHIP = -3,     /* a HIP runtime call or kernel launch failed */
    MQ_ENOMEM = -4,   /* device allocation failed */
    MQ_ECAP = -5      /* output capacity exceeded (join) */
};

/* Aggregates returned by the reductions (device-resident, 32 bytes). */
typedef struct mq_agg {
    uint64_t count;   /* rows that matched */
    int64_t sum;      /* exact int64 sum of the matched int32 values (query.c:325-354) */
    int32_t min;      /* INT32_MAX when count == 0 */
    int32_t max;      /* INT32_MIN when count == 0 */
    uint64_t _pad;
} mq_agg;

/* ---- runtime ---- */
int mq_init(int device);                 /* select/initialise a device; idempotent */
int mq_device_count(void);
const char* mq_last_error(void);
const char* mq_version(void);
int mq_malloc(void** dptr, size_t bytes);
int mq_free(void* dptr);
int mq_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int mq_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
/* D2H through the library's pinned staging buffers (synchronous): dst is never
 * registered with the driver, so it can be write-protected afterwards without
 * stalling later GPU work (a direct pageable D2H followed by mprotect does). */
int mq_memcpy_d2h_staged(void* dst, const void* src, size_t bytes, void* stream);
/* Start populating the fresh host pages of [p, p + bytes) in the background (helper
 * threads of the calling thread, MADV_POPULATE_WRITE: content unchanged). The next
 * mq_memcpy_d2h_staged into exactly that range copies each chunk as soon as its pages
 * are in; it also starts this itself when nothing covers its range. Callers that know
 * a result's size before its kernel runs start it first, so the page faults overlap
 * the kernel. MQ_PREFAULT=0 disables it, MQ_FAULT_THREADS (default 6) sizes it; the
 * staged copies' host memcpy runs on MQ_COPY_THREADS threads (default 6: the calling
 * thread and 5 helpers). */
void mq_host_prefault(void* p, size_t bytes);
/* Wait until the calling thread's population job (if any) has finished: call it
 * before freeing a range handed to mq_host_prefault that no staged copy consumed. */
void mq_host_prefault_wait(void);
int mq_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);
int mq_memset(void* dptr, int value, size_t bytes, void* stream);
int mq_stream_sync(void* stream);
void* mq_default_stream(void);
/* A non-blocking stream of its own on the calling thread's current device. */
int mq_stream_create(void** stream);
int mq_stream_destroy(void* stream);
/* Release the device scratch libmq keeps cached between calls (join tables and
 * partition buffers, probe arrays); the next call allocates afresh. */
void mq_trim(void);
/* Free the calling thread's pinned host staging buffers (the staged D2H/H2D ring
 * and shared_select's upload staging) on every device. A thread that stops using
 * libmq calls it before it exits (the row-shard workers do); later staged copies
 * on the thread allocate afresh. */
void mq_thread_release(void);
/* The same caching allocator for callers (the query layer keeps result shadows
 * and column copies in it). mq_pool_free hands the block out again at once, so it
 * frees only what no queued work still uses; mq_pool_free_on is the stream-ordered
 * free: the block is reused only after the work queued on `stream` so far has
 * finished (an event recorded on it; an allocation meanwhile gets a fresh block and
 * waits for the event only when no fresh block fits in HBM), so a caller frees right
 * after queueing the last kernel that reads it, with no host sync. Both also accept pointers from mq_malloc (freed at once;
 * mq_pool_free_on syncs the stream first). Call mq_pool_free_on with the block's
 * device current. */
int mq_pool_malloc(void** dptr, size_t bytes);
int mq_pool_free(void* dptr);
int mq_pool_free_on(void* dptr, void* stream);
/* Wait for all work queued on the calling thread's current device, on every stream
 * including the null stream (hipDeviceSynchronize). */
int mq_device_sync(void);

/* Workspace (device bytes) needed by the scan entry points for n rows. */
size_t mq_scan_workspace_bytes(uint64_t n);
/* The library's grid for a scan of n rows: blocks launched and rows per block. */
void mq_scan_geometry(uint64_t n, uint32_t* blocks, uint64_t* rows_per_block);
/* The fixed grids of the chunked passes, from the helpers their launches call; both need
 * no device, and any output pointer may be NULL. A block walks its chunk in steps (1024
 * rows, 256 bitmap words) and carries state from one step to the next.
 * group sort path (k_group_heads, k_group_seg_write) over n rows: blocks launched and
 * the rows in a block's chunk. */
void mq_group_sort_geometry(uint64_t n, uint32_t* blocks, uint64_t* chunk_rows);
/* delete / insert over n rows (an insert: n old + k new): the word prefix of the plan
 * (k_dml_word_sums, k_dml_word_prefix: blocks, bitmap words a chunk) and the index pass
 * of mq_delete_index (k_dml_index_count, k_dml_index_write: blocks, entries a chunk). */
void mq_dml_geometry(uint64_t n, uint32_t* prefix_blocks, uint64_t* prefix_chunk_words,
                     uint32_t* index_blocks, uint64_t* index_chunk_rows);
/* Test hook (no reference counterpart; as mq_shard_join_inject_failure in mq_query.h):
 * size every grid as on a device of at most `cus` compute units, so that a column of a
 * few million rows gives each block and wave the long row runs of a 1e9-row column.
 * cus > 0: every device, initialised already or later, counts min(its CUs, cus);
 * cus == 0: the hardware counts again (kept aside, no second device query);
 * cus < 0: MQ_EINVAL. The count is only ever lowered: kernels that wait for
 * lower-numbered blocks need the whole grid resident at once. The caller guarantees
 * that no libmq work is in flight and that no other thread is inside libmq; workspace
 * sizes that depend on the grid (mq_shared_select_workspace_bytes) are queried after
 * the call. Off by default, and no environment variable sets it. */
int mq_test_set_cu_limit(int cus);
/* Test hook: what a join handle (mq_join_build below) and its last probe and write are in,
 * so that a test can assert the path it means to compare before it compares. Host only:
 * it launches no kernel and changes nothing; with MQ_JOIN_STATE_ROW_WRITE set it waits for
 * the handle's stream and reads one word back. out (host, MQ_JOIN_STATE_WORDS u32):
 *   out[0]  the build's form: 1 = the unique table {key, build position}; 2 = a runs table
 *           (distinct keys -> run) or the partitioned words answering duplicate keys;
 *           0 = the global-CAS table of run heads;
 *   out[1]  MQ_JOIN_STATE_* flags;
 *   out[2]  with MQ_JOIN_STATE_ROW_WRITE: the entries (one per 65 536-pair chunk of a run
 *           of more than 4096 pairs) the last write listed for k_join_write_long; else 0. */
#define MQ_JOIN_STATE_WORDS 3
#define MQ_JOIN_STATE_PART 1u       /* the build kept its window partition (no global table) */
#define MQ_JOIN_STATE_DUPW 2u       /* ... and answers duplicate keys window by window */
#define MQ_JOIN_STATE_PACKED 4u     /* runs table: payloads are start << 4 | length */
#define MQ_JOIN_STATE_RS 8u         /* runs table over the sorted build (run bounds kept) */
#define MQ_JOIN_STATE_PRUNS 16u     /* last probe: a packed run per row, lengths per 64 rows */
#define MQ_JOIN_STATE_RUN2 32u      /* last probe: short runs' build positions per row */
#define MQ_JOIN_STATE_DEFERRED 64u  /* last probe: its last inverse pass is still to run */
#define MQ_JOIN_STATE_ROW_WRITE 128u /* the last write since that probe was the per-row one */
struct mq_join;
int mq_join_state(const struct mq_join* join, uint32_t* out);

/* ---- synthetic data (bench/tests; SURVEY.md §8(c) generator) ---- */
/* out[i] = (int32)(sm64(seed*0x100000001B3 + i) % modulus) */
int mq_gen_uniform(int32_t* d_out, uint64_t n, uint64_t seed, uint64_t modulus, void* stream);
/* hash-join keys of SURVEY §8(c) config 5 (kind 0 = build mix31(i), 1 = probe) and its
 * many-to-many variant (2 = build mix31(i mod n/2): every key twice; 3 = probe
 * mix31(sm64((7<<40)|j) mod n), n a power of two: about half hit), and iota */
int mq_gen_join_keys(int32_t* d_out, uint64_t n, int kind, void* stream);
int mq_gen_iota(int32_t* d_out, uint64_t n, void* stream);

/* ---- S1/S7 fused, one launch: count + int64 sum of rows of d_col in range ----
 * (select_column -> fetch_column -> sum, query.c:92-137 + 223-243 + 325-354, with
 * the positions never materialised). min/max are left INT32_MAX / INT32_MIN.
 * This is the bench's headline step. d_ws: >= mq_scan_workspace_bytes(0). */
int mq_select_sum(const int32_t* d_col, uint64_t n, int has_low, int32_t low, int has_high,
                  int32_t high, mq_agg* d_out, void* d_ws, size_t ws_bytes, void* stream);

/* ---- S1/S7 fused: count + int64 sum (+min/max) of rows of d_col in range ----
 * One HBM pass over d_col (4n bytes). *d_out receives the aggregate. */
int mq_select_agg(const int32_t* d_col, uint64_t n, int has_low, int32_t low, int has_high,
                  int32_t high, mq_agg* d_out, void* d_ws, size_t ws_bytes, void* stream);

/* The two launches of mq_select_agg, for callers that time the scan kernel alone:
 * mq_select_partials writes one partial per block into d_ws (and *nblocks);
 * mq_combine_partials folds nblocks partials from d_ws into *d_out.
 * want_minmax = 0 computes count + sum only (select + sum; min/max left at
 * INT32_MAX / INT32_MIN), 1 also min/max. */
int mq_select_partials(const int32_t* d_col, uint64_t n, int has_low, int32_t low, int has_high,
                       int32_t high, int want_minmax, void* d_ws, size_t ws_bytes,
                       uint32_t* nblocks, void* stream);
int mq_combine_partials(const void* d_ws, uint32_t nblocks, mq_agg* d_out, void* stream);

/* Diagnostic (no reference counterpart): the achievable HBM read rate for the
 * scan's access pattern (SURVEY.md §8(d) "achievable peak"). Streams d_col with
 * k_scan's loads and no predicate; *bytes_read receives the bytes the launch reads
 * (whole 8192-row groups of each block's chunk). d_ws: >= 8192 * 4 bytes. */
int mq_stream_read(const int32_t* d_col, uint64_t n, void* d_ws, size_t ws_bytes,
                   uint64_t* bytes_read, void* stream);

/* Diagnostic (no reference counterpart): the random-access ceiling of the join
 * probe. n_reads 8-byte reads of d_table (2^slots_log2
 * u64 slots) at hashed slots, 8 per lane in flight: k_ht_probe_unique's pattern
 * without the key compare or the output. d_ws: >= 8 bytes. */
int mq_random_read(const uint64_t* d_table, int slots_log2, uint64_t n_reads, void* d_ws, void* stream);

/* ---- J4 hashset.c (src/hashset.c:11-65) on the device ----
 * The set is the reference's own table: `size` int32 slots, 0 = empty, a key's
 * linear probe starting at hash(key, size) = key % size (multimap.c:60-63; a
 * negative key, an out-of-bounds index in the reference, starts at the wrapped
 * remainder here).
 * mq_hashset_lookup: d_found[i] = lookup_hashset(set, d_probe[i]) (hashset.c:35-45)
 *   for n probes; a full table without the key answers 0 after one lap (the
 *   reference loops forever).
 * mq_hashset_elements: the nonzero slots in slot order (get_hashset_elements,
 *   hashset.c:48-65) into d_out (capacity size); *d_count (device) receives their
 *   number. d_ws: mq_scan_workspace_bytes(size) bytes. */
int mq_hashset_lookup(const int32_t* d_table, int32_t size, const int32_t* d_probe, uint64_t n,
                      uint8_t* d_found, void* stream);
int mq_hashset_elements(const int32_t* d_table, uint64_t size, int32_t* d_out, uint64_t* d_count,
                        void* d_ws, size_t ws_bytes, void* stream);
/* mq_hashset_insert: the bulk form of insert_hashset (hashset.c:25-32). d_table holds
 *   `size` slots, all zero or left by earlier inserts; afterwards it holds exactly the
 *   slots that `for i in 0..n-1: insert_hashset(set, d_keys[i])` leaves: key 0 is never
 *   stored, a repeated key keeps its first place, and a key that finds no free slot in
 *   one lap is dropped (the reference loops forever). The layout does not depend on
 *   how the blocks are scheduled: the build is a linear probe ordered by first
 *   occurrence over a 64-bit working copy of the table. *d_stored
 *   (device, may be NULL) receives the number of nonzero slots afterwards. d_ws:
 *   mq_hashset_insert_workspace_bytes(size, n) bytes (8 per slot, and 8 per slot of a
 *   scratch table of the first power of two >= 2n slots). Asynchronous on `stream`.
 *   n == 0 leaves the table untouched. MQ_EINVAL for size <= 0, a NULL table, NULL keys
 *   with n > 0, n >= 2^32 - 1 or a short workspace. Keys that share one home slot cost
 *   O(n^2) probe steps, as in the reference. */
size_t mq_hashset_insert_workspace_bytes(uint64_t size, uint64_t n);
int mq_hashset_insert(int32_t* d_table, int32_t size, const int32_t* d_keys, uint64_t n,
                      uint64_t* d_stored, void* d_ws, size_t ws_bytes, void* stream);

/* Config-3 fused: aggregate of d_val[i] over rows i where d_sel[i] is in range. */
int mq_select_fetch_agg(const int32_t* d_sel, const int32_t* d_val, uint64_t n, int has_low,
                        int32_t low, int has_high, int32_t high, mq_agg* d_out, void* d_ws,
                        size_t ws_bytes, void* stream);

/* ---- S1 select_column_scan / S4 select_result: ordered compaction ----
 * Writes, in ascending i, d_payload ? d_payload[i] : i for every i whose d_col[i]
 * is in range, into d_pos_out (capacity n). *d_count receives K.
 * n must be < 2^31 (positions are int32, query.c:94). */
int mq_select_positions(const int32_t* d_col, const int32_t* d_payload, uint64_t n, int has_low,
                        int32_t low, int has_high, int32_t high, int32_t* d_pos_out,
                        uint64_t* d_count, void* d_ws, size_t ws_bytes, void* stream);

/* The same over a row shard: the rows are d_col[0..n) but number from row_base, so
 * without a payload the positions written are row_base + i (a column split into row
 * ranges across devices concatenates its shards' outputs in shard order).
 * row_base + n must be < 2^31. */
int mq_select_positions_at(const int32_t* d_col, const int32_t* d_payload, uint64_t n, int32_t row_base,
                           int has_low, int32_t low, int has_high, int32_t high, int32_t* d_pos_out,
                           uint64_t* d_count, void* d_ws, size_t ws_bytes, void* stream);

/* select_column's download pipeline (the API path): the ordered positions
 * of d_col[0..n) selected in `segs` contiguous row segments (1..64) queued on `stream`,
 * and each segment's positions downloaded into h_dst as soon as ITS kernel has finished,
 * through the staged D2H on a copy stream of the calling thread, while the later
 * segments' kernels still run. h_dst must hold n int32 (the caller's payload; untouched
 * beyond the K written). d_pos (capacity n) receives segment s's positions from its
 * first row (d_pos[r_s ...], r_s = h_rows[s]); h_seg[s] receives segment s's count and
 * h_rows[s] its first row (segs + 1 entries, h_rows[segs] = n). Returns when every
 * download is complete; the segments' positions in h_dst are contiguous in order. */
int mq_select_positions_download(const int32_t* d_col, uint64_t n, int has_low, int32_t low, int has_high,
                                 int32_t high, int segs, int32_t* d_pos, int32_t* h_dst, uint64_t* h_seg,
                                 uint64_t* h_rows, void* d_ws, size_t ws_bytes, void* stream);

/* ---- S6 select_column_sorted_index (query.c:143-198) ----
 * d_values: n int32 sorted ascending; d_positions: n size_t row ids. Restates the
 * reference's binary_search + run adjustment exactly (including its low == high
 * quirk), writes the run's positions (as int32) to d_pos_out, K to *d_count.
 * A bound below d_values[0], where the reference reads out of bounds, is defined: such a
 * low starts the run at row 0, such a high selects nothing. Calls queued on different
 * streams are independent (each takes its own scratch from the stream-ordered pool).
 * k_index_bounds walks a run of `low` / `high` on a single lane, one dependent load per
 * step. Nobody has measured what a long run costs. */
int mq_index_select(const int32_t* d_values, const uint64_t* d_positions, uint64_t n, int32_t low,
                    int32_t high, int32_t* d_pos_out, uint64_t* d_count, void* stream);

/* ---- index build (index.c:89-143) ----
 * Sorted copy of d_col (n < 2^32 rows): d_values_out ascending (may be NULL) and
 * d_positions_out[i] (size_t, may be NULL) the row it came from, equal values in
 * ascending row order. (The reference's quicksort orders equal values its own way;
 * the values, and the positions of distinct values, are identical.) */
int mq_index_build(const int32_t* d_col, uint64_t n, int32_t* d_values_out,
                   uint64_t* d_positions_out, void* stream);
/* The same in the reference quicksort's own order (index.c:25-46), equal values
 * included: a level-synchronous restatement of the Lomuto recursion (n < 2^31).
 * Costs a few passes over n per recursion depth (O(log n) depths on distinct-ish
 * data; a range of equal values finishes in one). */
int mq_index_build_lomuto(const int32_t* d_col, uint64_t n, int32_t* d_values_out,
                          uint64_t* d_positions_out, void* stream);
/* The build_index drop-in's policy: the radix sort; if the values hold ties and
 * n <= exact_max, the Lomuto order instead (distinct values have one order, so the
 * radix result is already the reference's). *h_exact = 0 when ties were left in
 * ascending row order (n > exact_max). d_values_out is required. */
int mq_index_build_ref(const int32_t* d_col, uint64_t n, int32_t* d_values_out, uint64_t* d_positions_out,
                       uint64_t exact_max, int* h_exact, void* stream);
/* reorder_column (index.c:105-114): d_out[i] = d_col[d_positions[i]] (size_t positions) */
int mq_gather_u64(const int32_t* d_col, const uint64_t* d_positions, uint64_t n, int32_t* d_out,
                  void* stream);
/* build_histogram's counts (index.c:63-84): d_counts[b] (101 u64) = rows with
 * (int)(v - col_min) / bin_size == b for b in [0, 100); d_counts[100] = rows outside
 * (the reference writes those past its 100-entry array). bin_size != 0. */
int mq_histogram(const int32_t* d_col, uint64_t n, int32_t col_min, int32_t bin_size,
                 uint64_t* d_counts, void* stream);

/* ---- row deletes and updates by a position list ----
 * The write path behind relational_delete / relational_update (mq_query.h). The
 * reference has no such operator (its parser lacks both commands); the semantics are
 * its workload generator's (milestone5.py:127-142, 186-202): a delete drops the listed
 * rows from every column of a table and the survivors keep their order, an update
 * assigns one value to the listed rows of one column. A delete is a plan and two apply
 * steps on one workspace of mq_delete_workspace_bytes(n) bytes (16-byte aligned):
 * plan:    d_pos holds k int32 row ids of a table of n < 2^31 rows, in any order,
 *          repeats allowed. Builds one bit per row and the count of deleted rows before
 *          each 64-bit word of them. Synchronises; *h_deleted = distinct rows marked,
 *          *h_bad = ids outside [0, n). With *h_bad != 0 it returns MQ_EINVAL and leaves
 *          no plan. k == 0 is a valid plan that deletes nothing.
 * columns: d_out[j] (capacity n - deleted) receives the surviving rows of d_cols[j] in
 *          ascending row order, for ncols <= 1024 columns; d_cols / d_out are host arrays
 *          of device pointers, d_out[j] != d_cols[j]. Per column 4n bytes read,
 *          4(n - deleted) written and 3n/16 of bitmap and word counts.
 * index:   a sorted index over the same n rows (d_values ascending, d_positions size_t
 *          row ids, a permutation of the rows: the identity for a clustered index):
 *          the entries whose row survives, in their order, each position p renumbered
 *          to p - (deleted rows before p). Either output may be NULL only when nothing
 *          survives. Its temporaries live in the workspace.
 * Both apply steps run on the plan the calling thread made last, on that workspace and
 * device, are asynchronous on `stream`, and may be repeated (other columns, other
 * indexes) while the workspace is untouched.
 * mq_update_rows: d_col[d_pos[i]] = value for every id in [0, n); ids outside are
 *          skipped and *d_bad (device, may be NULL) receives their number. Repeated ids
 *          are harmless. Asynchronous on `stream`.
 * MQ_EINVAL: NULL pointers, n >= 2^31, a short or misaligned workspace, no plan. */
size_t mq_delete_workspace_bytes(uint64_t n);
int mq_delete_plan(const int32_t* d_pos, uint64_t k, uint64_t n, uint64_t* h_deleted,
                   uint64_t* h_bad, void* d_ws, size_t ws_bytes, void* stream);
int mq_delete_columns(const void* d_ws, const int32_t* const* d_cols, int ncols,
                      int32_t* const* d_out, void* stream);
int mq_delete_index(void* d_ws, const int32_t* d_values, const uint64_t* d_positions,
                    int32_t* d_values_out, uint64_t* d_positions_out, void* stream);
int mq_update_rows(int32_t* d_col, uint64_t n, const int32_t* d_pos, uint64_t k, int32_t value,
                   uint64_t* d_bad, void* stream);

/* ---- batched row inserts ----
 * The write path behind relational_insert (mq_query.h): the inverse of the delete. k new
 * rows are interleaved with n old ones (n + k < 2^31); the j-th new row, in insertion
 * order, goes in front of old row d_ins[j] (after the last one when d_ins[j] = n), and
 * new rows with equal points keep their order. A plan and two apply steps on one
 * workspace of mq_insert_workspace_bytes(n, k) bytes (16-byte aligned):
 * points:  d_ins[j] (u32) = the entries of the ascending d_sorted[0, n) that are <=
 *          d_new_sorted[j], by binary search: where a new key goes so that it follows
 *          every old key <= it. Ascending new keys give ascending points.
 * plan:    one bit per output slot, set for slot d_ins[j] + j (the j-th new row's), and
 *          the count of set bits before each 64-bit word. Synchronises; *h_bad = points
 *          that exceed n or lie below the point before them. With *h_bad != 0 it returns
 *          MQ_EINVAL and leaves no plan. k == 0 is a valid plan that inserts nothing.
 * columns: d_out[j][s] = bit(s) ? d_new[j][rank1(s)] : d_old[j][s - rank1(s)] for every
 *          slot s < n + k, rank1(s) the set bits below s; d_new[j] holds the column's k new
 *          values in insertion order; ncols <= 1024; d_old / d_new / d_out are host
 *          arrays of device pointers, 4-byte aligned, d_out[j] distinct from both inputs.
 *          Per column 4n + 4k bytes read, 4(n + k) written and 3(n + k)/16 of bitmap and
 *          word counts.
 * index:   the same expansion over a sorted index (int32 values, size_t positions) with
 *          the new entries (d_new_values ascending, d_new_positions their rows) of a plan
 *          made from the index's own points. With d_renumber_ins (k_renumber ascending
 *          u32 points of the TABLE's interleave; NULL / 0 for an append) every old
 *          position p becomes p + #{j : d_renumber_ins[j] <= p}, the row's new slot.
 * slots:   d_slots[d_order ? d_order[j] : j] = d_ins[j] + j, the slot of every new row
 *          filed under its batch index (d_order: the permutation that sorted the batch,
 *          mq_index_build's positions; an entry outside [0, k) files nothing).
 * positions: d_out[i] = d_slots ? d_slots[d_order[i]] : base + d_order[i]: the rows of the
 *          batch entries in another sorted order (an unclustered index's new entries).
 * The apply steps run on the insert plan the calling thread made last, on that workspace
 * and device, are asynchronous on `stream`, and may be repeated while the workspace is
 * untouched (a delete plan on the same workspace ends the insert plan, and the reverse).
 * MQ_EINVAL: NULL pointers, n + k >= 2^31, a short or misaligned workspace, no plan. */
size_t mq_insert_workspace_bytes(uint64_t n, uint64_t k);
int mq_insert_points(const int32_t* d_sorted, uint64_t n, const int32_t* d_new_sorted, uint64_t k,
                     uint32_t* d_ins, void* stream);
int mq_insert_plan(const uint32_t* d_ins, uint64_t k, uint64_t n, uint64_t* h_bad, void* d_ws,
                   size_t ws_bytes, void* stream);
int mq_insert_columns(const void* d_ws, const int32_t* const* d_old, const int32_t* const* d_new,
                      int ncols, int32_t* const* d_out, void* stream);
int mq_insert_index(const void* d_ws, const int32_t* d_values, const uint64_t* d_positions,
                    const int32_t* d_new_values, const uint64_t* d_new_positions,
                    const uint32_t* d_renumber_ins, uint64_t k_renumber, int32_t* d_values_out,
                    uint64_t* d_positions_out, void* stream);
int mq_insert_slots(const uint32_t* d_ins, const uint64_t* d_order, uint64_t k, uint64_t* d_slots,
                    void* stream);
int mq_insert_positions(const uint64_t* d_slots, uint64_t base, const uint64_t* d_order, uint64_t k,
                        uint64_t* d_out, void* stream);

/* ---- grouped aggregates by an int32 key ----
 * n < 2^31 rows of (d_keys[i], d_vals[i]) give one entry per distinct key, in ascending
 * signed key order: the key, its row count, the exact int64 sum of its values and their
 * min / max. The reference has no such operator. d_vals may equal d_keys. Integer adds,
 * mins and maxes only: the result is bitwise the same whatever the path, the grid or the
 * order in which blocks finish. A plan and a write on a handle:
 * plan:  h_key_bounds is NULL or a host {lo, hi} pair, inclusive, that may be wider than
 *        the keys; NULL costs one more read of the keys (mq_reduce). The key range
 *        hi - lo + 1 (64-bit: up to 2^32) picks the path under MQ_GROUP_AUTO: at most
 *        mq_group_dense_slots() takes the dense path (one streaming read of both columns,
 *        a table in LDS per block), anything wider the sort path (mq_index_build, then a
 *        segmented fold through the positions). Synchronises; *h_groups = the number of
 *        distinct keys, *h_path (may be NULL) the path taken. n == 0 gives zero groups.
 *        MQ_EINVAL, with *h_groups = 0 and *out = NULL: a key outside the given bounds,
 *        lo > hi with n > 0, MQ_GROUP_DENSE forced on a wider range, n >= 2^31, NULL or
 *        misaligned columns. d_vals must stay valid until the write has run.
 * write: the *h_groups entries into the outputs (capacity *h_groups each; nothing is
 *        written at or past it). Any of the pointers may be NULL: that output is not
 *        wanted. Asynchronous on `stream`, on the plan's device; may be repeated.
 * free:  releases the handle; its buffers are freed in the order of the stream that the
 *        last write was queued on. */
enum { MQ_GROUP_AUTO = 0, MQ_GROUP_DENSE = 1, MQ_GROUP_SORT = 2 };
typedef struct mq_group mq_group;
uint32_t mq_group_dense_slots(void);   /* a constant; needs no device */
int mq_group_plan(const int32_t* d_keys, const int32_t* d_vals, uint64_t n,
                  const int32_t* h_key_bounds, int path, mq_group** out,
                  uint64_t* h_groups, int* h_path, void* stream);
int mq_group_write(mq_group* g, int32_t* d_keys_out, uint64_t* d_count_out,
                   int64_t* d_sum_out, int32_t* d_min_out, int32_t* d_max_out,
                   void* stream);
int mq_group_free(mq_group* g);

/* ---- GROUP BY under a WHERE, in one pass ----
 * mq_group_plan over the rows for which a conjunction of range predicates holds: with
 * m[i] = every range holds for row i (d_cols, h_ranges and ncols as mq_where_positions takes
 * and defines them, further down in this header; the predicates are evaluated in the order
 * given, the most selective belongs first), the result is exactly that of mq_group_plan over
 * (d_keys[m], d_vals[m]): one entry per distinct key with a matching row, ascending, u64
 * count, exact int64 sum, min and max; bitwise the same whatever the path, the grid, the
 * order of the predicates or the alignment. The handle is an ordinary mq_group, served by
 * mq_group_write and mq_group_free. *h_rows (may be NULL) = the matching rows, the sum of the
 * counts. d_keys and d_vals may be each other or any predicate column.
 * h_key_bounds (NULL or a host {lo, hi}, inclusive) constrains the keys of MATCHING rows
 *        only: the key of a row that fails a predicate is never an error and never an
 *        address. NULL costs one more pass over the predicates and over the key lines that
 *        hold a survivor (mq_where_agg on the key column), which finds the range of the
 *        matching keys alone: a filter that narrows the keys to mq_group_dense_slots() values
 *        lands on the dense path whatever the column holds elsewhere. The range hi - lo + 1
 *        picks the path as in mq_group_plan; `path` forces one.
 * dense: one streaming pass, k_group_where_dense: the predicate columns as mq_where_agg
 *        reads them, then of the key and the value column only the 128-byte lines in which a
 *        row survived, into the per-block LDS tables of mq_group_plan's dense path.
 * sort:  mq_where_positions, the K matching rows' keys and values gathered (mq_fetch) into
 *        two buffers the handle owns or frees, then mq_group_plan's sort path on those; given
 *        bounds are checked against the sorted ends.
 * Measured at 1e9 rows against mq_where_positions -> mq_fetch x 2 ->
 * mq_group_plan with the same bounds: with bounds given 0.59-0.68 of the chain's time when
 * 10 % of the rows match and 0.24-0.41 at 100 %, a win at 0.1-1 % too behind a uniform leading
 * column but a loss there behind a clustered one (1.07-1.56; a few blocks do every table
 * update); with NULL bounds a win from 50 % upward (0.37-0.88), a tie at 10 % and a loss below
 * (1.2-2.3). Every range unbounded runs 3-5 % behind mq_group_plan. Nothing is dispatched
 * differently by selectivity.
 * Synchronises; takes its scratch from the library's pool. n == 0, a range that no int32
 * satisfies (no column is read) or no matching row give MQ_OK, zero groups and a handle to
 * free. d_vals must stay valid until the write has run (dense path).
 * MQ_EINVAL, with *out = NULL, *h_groups = 0 and nothing allocated: ncols outside 1..8,
 * n >= 2^31, a NULL d_cols, h_ranges, out or h_groups, a NULL or not 4-byte aligned column,
 * key or value pointer with n > 0, a path that is none of the three, lo > hi with n > 0; and
 * with everything released: a matching row whose key lies outside the given bounds,
 * MQ_GROUP_DENSE forced on a wider range. */
struct mq_range;
int mq_group_where_plan(const int32_t* const* d_cols /* host array of ncols device pointers */,
                        const struct mq_range* h_ranges, int ncols, const int32_t* d_keys,
                        const int32_t* d_vals, uint64_t n,
                        const int32_t* h_key_bounds /* NULL or {lo, hi} inclusive */, int path,
                        mq_group** out, uint64_t* h_groups, int* h_path /* may be NULL */,
                        uint64_t* h_rows /* matching rows; may be NULL */, void* stream);

/* ---- GROUP BY over two to four int32 key columns ----
 * nkeys key columns K_0 .. K_{nkeys-1} (nkeys in 1..MQ_GROUP_MAX_KEYS) and one value column,
 * each n < 2^31 int32 rows, give one entry per distinct tuple (K_0[i], .., K_{nkeys-1}[i]), in
 * ascending lexicographic order (K_0 the most significant, every component as signed int32):
 * the tuple, its u64 row count, the exact int64 sum of the values and their min / max.
 * Integer adds, mins and maxes only: bitwise the same whatever the path, the grid, the order
 * in which blocks finish or the alignment. Any two of the pointers may be the same column.
 * nkeys == 1 is mq_group_plan itself (the call is handed on). The handle is an ordinary
 * mq_group: mq_group_free releases it; mq_group_write on a handle with nkeys > 1 writes the
 * aggregates with d_keys_out == NULL and answers MQ_EINVAL otherwise (one column cannot hold
 * the tuple).
 * h_key_bounds is NULL (one mq_reduce per key column) or {lo_0, hi_0, lo_1, hi_1, ..}, inclusive,
 *        possibly wider than the keys. The key space P = prod(hi_j - lo_j + 1), in 64 bits,
 *        picks the path as the range does in mq_group_plan; mq_group_by_auto_path says which
 *        without a device.
 * dense (P <= mq_group_dense_slots()): one streaming read of the nkeys + 1 columns,
 *        k_group_by_dense, into mq_group_plan's per-block LDS tables at slot
 *        sum((K_j - lo_j) * stride_j), stride_{nkeys-1} = 1, stride_j = stride_{j+1} *
 *        range_{j+1}: slot order is the output order.
 * sort  (P <= 2^32): k_group_by_pack reads the key columns once and writes one int32 column of
 *        code ^ 0x80000000 (code = the same sum as a u32; P = 2^32 exactly works), then
 *        mq_group_plan's sort path on that column.
 * Every component is checked against its own bounds on both paths: a row with a key outside
 * its column's bounds is never an address and fails the plan (MQ_EINVAL, everything released),
 * also where the summed slot would lie inside the table.
 * write: as mq_group_write; d_keys_out is NULL or a host array of nkeys device pointers, any
 *        of them NULL. The groups' slots or codes go to a pooled temporary of *h_groups int32,
 *        freed in the stream's order, and k_group_by_unpack decodes them:
 *        K_j = lo_j + (code / stride_j) % range_j.
 * Measured at 1e9 rows, plan + write: dense with bounds 1.03-1.12 of
 * mq_stream_read over the nkeys + 1 columns (1.35 with 12 uniformly mixed tuples, LDS
 * collisions as in mq_group_plan), each NULL bound 0.6 ms more; the packed path 1.06-1.28 of
 * mq_group_plan's sort path on one prepacked column.
 * Synchronises (plan); n == 0 gives zero groups and a handle to free. MQ_EINVAL, with
 * *out = NULL, *h_groups = 0 and nothing allocated: nkeys outside 1..4, NULL or not 4-byte
 * aligned columns with n > 0, a NULL out or h_groups, n >= 2^31, a path that is none of the
 * three, lo_j > hi_j with n > 0, P > 2^32, MQ_GROUP_DENSE forced on
 * P > mq_group_dense_slots(). MQ_GROUP_SORT may be forced for any P <= 2^32. */
enum { MQ_GROUP_MAX_KEYS = 4 };
/* needs no device: MQ_GROUP_DENSE, MQ_GROUP_SORT, or MQ_EINVAL (nkeys outside 1..4, a lo > hi,
 * or a key space wider than 2^32); *h_space (may be NULL) = prod(hi_j - lo_j + 1), saturated at 2^63 */
int mq_group_by_auto_path(const int32_t* h_key_bounds /* {lo0,hi0,lo1,hi1,...} inclusive */, int nkeys,
                          uint64_t* h_space);
int mq_group_by_plan(const int32_t* const* d_keys /* host array of nkeys device pointers */, int nkeys,
                     const int32_t* d_vals, uint64_t n,
                     const int32_t* h_key_bounds /* NULL or 2*nkeys host ints */, int path,
                     mq_group** out, uint64_t* h_groups, int* h_path /* may be NULL */, void* stream);
int mq_group_by_write(mq_group* g, int32_t* const* d_keys_out /* NULL, or host array of nkeys device
                      pointers, any of them NULL */, uint64_t* d_count_out, int64_t* d_sum_out,
                      int32_t* d_min_out, int32_t* d_max_out, void* stream);

/* ---- GROUP BY over two to four key columns under a WHERE ----
 * SELECT k0, k1, .., count(*), sum(v), min(v), max(v) WHERE c0 IN [..) AND .. GROUP BY k0, k1, ..
 * in one operator. With m[i] = every one of the ncols ranges holds for row i
 * (mq_group_where_plan's predicates), the result is exactly that of mq_group_by_plan over the
 * key columns and the values restricted to m; bitwise the same whatever the path, the grid, the
 * alignment, the order of the predicates or the order in which blocks finish. The handle is an
 * ordinary mq_group with nkeys > 1, served by mq_group_by_write and mq_group_free. *h_rows (may
 * be NULL) = the matching rows. Any of the pointers may be the same column, a key a predicate
 * column and the values a key among them. nkeys == 1 is mq_group_where_plan itself (the call is
 * handed on).
 * h_key_bounds (NULL or {lo_0, hi_0, lo_1, hi_1, ..}, inclusive) constrains the components of
 *        MATCHING rows only: a component of a row that fails a predicate is never an error and
 *        never an address. Every component of a matching row is checked against its own
 *        column's bounds (mq_group_by_plan's rule: (3, 12) under ranges (10, 10) fails though its
 *        summed code lies inside the table). NULL costs one more pass, k_group_by_where_bounds:
 *        the predicates and the surviving key lines of all nkeys columns at once give every
 *        column's min and max over the matching rows and their number. P = prod(hi_j - lo_j + 1)
 *        picks the path as in mq_group_by_plan (mq_group_by_auto_path says which).
 * dense (P <= mq_group_dense_slots()): one streaming pass, k_group_by_where_dense: the predicate
 *        columns as mq_where_agg reads them, then of the nkeys key columns and the value column
 *        only the 128-byte lines in which a row survived, the tuple's code as the slot of
 *        mq_group_plan's per-block LDS tables.
 * sort  (P <= 2^32): mq_where_positions, then k_group_by_pack_pos writes code ^ 0x80000000 of
 *        the K matching rows straight from the key columns through the positions (no key column
 *        is gathered), the values are gathered (mq_fetch) into a buffer the handle owns, and
 *        mq_group_plan's sort path runs on the packed column.
 * Measured at 1e9 rows (nkeys 2 and 4 over 2025 tuples, a leading predicate
 * that passes 0.1-100 % of its column and a second one that passes half) against
 * mq_where_positions -> mq_fetch x (nkeys + 1) -> mq_group_by_plan with the same bounds: with
 * bounds given, behind a uniform leading column 0.81-0.87 of the chain's time at 0.1 %, a tie
 * at 1 % (1.01-1.04), 0.68-0.69 at 10 %, 0.48-0.51 at 50 % and 0.36-0.39 at 100 %; behind a
 * clustered one 0.91-0.98 at 10 %, 0.35-0.45 from 50 % upward and a loss at 0.1-1 % (1.48-1.72;
 * a few blocks do every table update); with NULL bounds a win from 50 % upward (0.59-0.86) and
 * a loss below (1.21-1.63 uniform, 1.32-2.58 clustered). Every range unbounded runs 0-3 %
 * behind mq_group_by_plan. The sort path with 1e8 matching rows in 6.3e7 groups: 0.90-0.94 of
 * the chain. Nothing is dispatched differently by selectivity.
 * Synchronises; takes its scratch from the library's pool. n == 0, a range that no int32
 * satisfies (no column is read) or no matching row give MQ_OK, zero groups and a handle to
 * free. d_vals must stay valid until the write has run (dense path).
 * MQ_EINVAL, with *out = NULL, *h_groups = 0, *h_rows = 0 and nothing allocated: ncols outside
 * 1..8, nkeys outside 1..4, n >= 2^31, a NULL d_cols, h_ranges, d_keys, out or h_groups, a NULL
 * or not 4-byte aligned column, key or value pointer with n > 0, a path that is none of the
 * three, and of given bounds with n > 0 lo_j > hi_j, P > 2^32, MQ_GROUP_DENSE forced on
 * P > mq_group_dense_slots(); with everything released: a matching row with a component outside
 * its column's given bounds, and P > 2^32 or a forced MQ_GROUP_DENSE past the slots for the
 * bounds the plan found. */
int mq_group_by_where_plan(const int32_t* const* d_cols /* host array of ncols device pointers */,
                           const struct mq_range* h_ranges, int ncols,
                           const int32_t* const* d_keys /* host array of nkeys device pointers */, int nkeys,
                           const int32_t* d_vals, uint64_t n,
                           const int32_t* h_key_bounds /* NULL or 2*nkeys host ints */, int path,
                           mq_group** out, uint64_t* h_groups, int* h_path /* may be NULL */,
                           uint64_t* h_rows /* matching rows; may be NULL */, void* stream);

/* ---- top k: the k smallest or largest rows, in order ----
 * n < 2^31 int32 values d_vals[i] with an optional int32 payload d_payload[i] (a positions
 * vector, the pair select_result takes; NULL: the payload is the row id i). The output is
 * m = min(k, n) pairs (value, payload): ascending, the m smallest values in ascending
 * order; descending (descending != 0), the m largest in descending order; equal values by
 * ascending input index i in both directions. That is the first m entries of a stable sort
 * (numpy: argsort(v, kind="stable")[:m], of ~v for descending), so the result is unique and
 * bitwise the same on every path and grid. The reference has no such operator.
 * select: a radix select. Each value maps to a u32 key in output order (sign bit flipped,
 *        complemented for descending). One streaming read counts the key's top 11 bits into
 *        2048 bins; the bin that holds the m-th key is the boundary. While it holds more
 *        than cand_cap rows the read is repeated over its rows alone for the next 11 bits,
 *        then the last 10 (at most three reads: h_info->levels). One more read collects, in
 *        input order, every row before the boundary prefix and the rows on it: all of them
 *        when they fit cand_cap, else (the prefix is one value by then) only the first
 *        m - (rows before) of them. The candidates, at most k + cand_cap, go through
 *        mq_index_build and the first m are gathered. Workspace O(k + cand_cap + blocks).
 * sort:  mq_index_build of the whole column (of ~v for descending), the first m gathered.
 * MQ_TOPK_AUTO takes the sort path when min(k, n) + cand_cap > n / MQ_TOPK_SORT_DIV (so
 * many candidates that selecting them saves nothing; mq_topk_auto_path answers the rule
 * and needs no device), else the select path; MQ_TOPK_SELECT / MQ_TOPK_SORT force one for
 * any k. cand_cap == 0 means mq_topk_default_cap().
 * Synchronises (the host picks the boundary between the reads). Either output may be NULL;
 * nothing is written at or past entry m. k == 0 or n == 0 gives m = 0 and MQ_OK.
 * MQ_EINVAL, with nothing written: n >= 2^31, a NULL (n > 0) or misaligned (not 4-byte)
 * d_vals or d_payload, a path that is none of the three. */
enum { MQ_TOPK_AUTO = 0, MQ_TOPK_SELECT = 1, MQ_TOPK_SORT = 2 };
enum { MQ_TOPK_SORT_DIV = 4 };
typedef struct mq_topk_info {
    uint64_t m;           /* entries written: min(k, n) */
    uint64_t candidates;  /* entries handed to the final sort (sort path: n) */
    uint64_t ties;        /* rows equal to the threshold value (entry m - 1) that were left out */
    int32_t  path;        /* MQ_TOPK_SELECT or MQ_TOPK_SORT */
    int32_t  levels;      /* histogram passes over the column (select path: 1..3; sort path: 0) */
} mq_topk_info;
uint64_t mq_topk_default_cap(void);   /* a constant; needs no device */
int mq_topk_auto_path(uint64_t n, uint64_t k, uint64_t cand_cap /* 0: default */);
int mq_topk(const int32_t* d_vals, const int32_t* d_payload /* may be NULL */, uint64_t n,
            uint64_t k, int descending, int path, uint64_t cand_cap /* 0: default */,
            int32_t* d_vals_out, int32_t* d_payload_out, mq_topk_info* h_info /* may be NULL */,
            void* stream);

/* ---- HAVING, ORDER BY an aggregate and LIMIT: top k over int64 entries ----
 * n < 2^31 entries. Entry i passes when d_having is NULL or h_having (low <= v < high, either
 * bound optional) holds for d_having[i]. The output is the first m = min(k, passed) passing
 * entries of a stable sort by d_vals[i], as pairs (value, index i): ascending, the smallest
 * first; descending (descending != 0), the largest first, that is a stable sort by ~v; equal
 * values in ascending i in both directions (numpy: idx = flatnonzero(mask);
 * idx[argsort(v[idx], kind="stable")][:k], of ~v[idx] for descending). With d_vals == NULL the
 * order is i itself, whatever `descending` says: an ordered compaction of the passing entries
 * cut at k (HAVING alone, in key order), and d_vals_out receives the index as an int64; both
 * paths are then one counting read and the collect (candidates = m, ties = 0, levels = 1 on
 * the select path).
 * d_having may equal d_vals. The result is unique, so it is bitwise the same on every path,
 * grid and cand_cap. The reference has no such operator.
 * select: §3.12's radix select on 64-bit keys. Each value maps to a u64 in output order (sign bit
 *        flipped, complemented for descending; mq_topk64_key). One streaming read, 16-byte loads,
 *        counts the passing entries' top 11 key bits into 2048 LDS bins a block; with a filter
 *        column of its own the value is requested only for a wave tile (256 entries) in which an
 *        entry passed. While the boundary bin holds more than cand_cap entries the read repeats
 *        over that prefix alone for the next digit (shifts 53, 42, 31, 20, 9, 0, the last digit 9
 *        bits: at most six reads, h_info->levels). One ordered collect read takes every passing
 *        entry before the boundary prefix and the entries on it: all of them when they fit
 *        cand_cap, else (the prefix is one value by then) the first m - (entries before). The
 *        candidates, at most k + cand_cap, are sorted by (key, index) with two stable
 *        mq_index_build runs (low word, then high word) and the first m gathered. Workspace
 *        O(k + cand_cap + blocks), from the pool.
 * sort:  one counting read, the passing entries compacted and all of them sorted the same way:
 *        ORDER BY without a LIMIT is k = UINT64_MAX.
 * MQ_TOPK_AUTO is mq_topk's rule with mq_topk's constants (mq_topk64_auto_path; needs no device):
 * sort when min(k, n) + cand_cap > n / MQ_TOPK_SORT_DIV. The constants have NOT been swept for
 * 64-bit entries. cand_cap == 0 means mq_topk_default_cap().
 * Synchronises, as mq_topk does. Either output may be NULL; nothing is written at or past entry
 * m. k == 0 or n == 0 gives m = 0 and MQ_OK. MQ_EINVAL, with nothing written: n >= 2^31, a
 * d_vals, d_having or d_vals_out that is not 8-byte aligned, a d_idx_out that is not 4-byte
 * aligned, d_having set with h_having NULL, a path that is none of the three.
 * mq_topk64_widen (d_out[i] = d_in[i], sign-extended) and mq_topk64_take (d_out[i] =
 * d_col[d_idx[i]], elements of 4 or 8 bytes) are the asynchronous helpers around it: a column of
 * int32 aggregates made sortable, and any column gathered through the indices. */
typedef struct mq_range64 { int has_low; int64_t low; int has_high; int64_t high; } mq_range64; /* low <= v < high */
typedef struct mq_topk64_info {
    uint64_t m;          /* entries written: min(k, passed) */
    uint64_t passed;     /* entries for which the filter holds (n without a filter) */
    uint64_t candidates; /* entries handed to the final sort (sort path: passed) */
    uint64_t ties;       /* passing entries equal to entry m-1's value that were left out */
    int32_t  path;       /* MQ_TOPK_SELECT or MQ_TOPK_SORT */
    int32_t  levels;     /* histogram reads (select path 1..6, sort path 0) */
} mq_topk64_info;
uint64_t mq_topk64_key(int64_t v, int descending);   /* host-callable; needs no device */
int mq_topk64_auto_path(uint64_t n, uint64_t k, uint64_t cand_cap /* 0: mq_topk_default_cap() */);
int mq_topk64(const int64_t* d_vals /* NULL: order by the entry's index */,
              const int64_t* d_having /* NULL: no filter */, const mq_range64* h_having,
              uint64_t n, uint64_t k, int descending, int path, uint64_t cand_cap,
              int64_t* d_vals_out /* may be NULL */, uint32_t* d_idx_out /* may be NULL */,
              mq_topk64_info* h_info /* may be NULL */, void* stream);
int mq_topk64_widen(const int32_t* d_in, uint64_t n, int64_t* d_out, void* stream);
int mq_topk64_take(const void* d_col, int elem_bytes /* 4 or 8 */, const uint32_t* d_idx, uint64_t m,
                   void* d_out, void* stream);

/* ---- the same on a group handle: HAVING, ORDER BY, LIMIT over its groups ----
 * g is an mq_group from mq_group_plan, _where_, _by_, _by_where_, _join_ or _star_plan. The
 * entries are its groups in key order (the order mq_group_write / mq_group_by_write give,
 * lexicographic tuples). The ordering aggregate o->order_by and the filter aggregate
 * o->having_by are materialised as int64 columns of `groups` entries (the handle's own write
 * into pool buffers; int32 min / max widened), mq_topk64 runs on them and every requested output
 * is gathered through its indices: ties in the ordering aggregate come in ascending key order, and
 * the result equals mq_group_by_write of everything followed by the numpy model above.
 * order_by == MQ_AGG_KEY keeps key order (HAVING and LIMIT only; `descending` is ignored);
 * having_by == MQ_AGG_KEY (0) means no HAVING. Output capacity min(k, groups) each; *h_m = the
 * entries written. d_keys_out is NULL or a host array of the handle's nkeys (>= 1) device
 * pointers, any of them NULL. The handle stays usable: mq_group_write still gives all groups,
 * and mq_group_top may be repeated with another order. Synchronises (mq_topk64 does). The device
 * check, the stream bookkeeping and groups == 0 (*h_m = 0, MQ_OK) are mq_group_write's.
 * MQ_EINVAL: an order_by or having_by that is no MQ_AGG_*, a NULL g, o or h_m, and mq_topk64's
 * own cases. mq_mgroup handles (mq_group_measures_plan) have no such form: their results go
 * through the drop-in group_top_k (mq_query.h). */
enum { MQ_AGG_KEY = 0, MQ_AGG_COUNT = 1, MQ_AGG_SUM = 2, MQ_AGG_MIN = 3, MQ_AGG_MAX = 4 };
typedef struct mq_group_order {
    int order_by;      /* MQ_AGG_*; MQ_AGG_KEY: key order, i.e. HAVING and LIMIT only */
    int descending;
    uint64_t k;        /* UINT64_MAX: no LIMIT */
    int having_by;     /* MQ_AGG_COUNT..MQ_AGG_MAX, or MQ_AGG_KEY (0): no HAVING */
    mq_range64 having;
    int path;          /* MQ_TOPK_* */
    uint64_t cand_cap; /* 0: default */
} mq_group_order;
int mq_group_top(mq_group* g, const mq_group_order* o, uint64_t* h_m,
                 int32_t* const* d_keys_out /* NULL, or host array of the handle's nkeys (>= 1) pointers, any NULL */,
                 uint64_t* d_count_out, int64_t* d_sum_out, int32_t* d_min_out, int32_t* d_max_out,
                 mq_topk64_info* h_info, void* stream);

/* ---- WHERE a IN [..) AND b IN [..) ...: a conjunctive range select ----
 * ncols (1 .. MQ_WHERE_MAX_COLS) columns of n < 2^31 int32 rows and one range per column:
 * row i matches when every range holds for it. A range is {has_low, low, has_high, high}
 * and means low <= v < high with either bound optional, as everywhere in this header.
 * d_cols is a HOST array of ncols device pointers, h_ranges a HOST array of ncols ranges;
 * the same column may appear more than once. The reference has no such operator: its DSL
 * spells a conjunction as the chain select -> fetch -> select_result -> fetch -> ...
 * positions: in ascending i, d_payload ? d_payload[i] : i of every matching row into
 *        d_pos_out (capacity n; nothing is written at or past entry K) and K into *d_count
 *        (device). With ncols == 1 that is mq_select_positions bit for bit; for any ncols it
 *        is what the chain returns.
 * agg:   {count, int64 sum, min, max} of d_val[i] over the matching rows into *d_out
 *        (device); with no match count and sum are 0, min INT32_MAX and max INT32_MIN, as
 *        mq_select_agg leaves them. d_val may be one of the predicate columns.
 * Every predicate column is streamed once at most; of column c + 1 only the 128-byte lines
 * (32 rows) in which predicates 0..c left a row are requested, so the predicates are
 * evaluated in the order given and libmq does not reorder them: the answer does not depend
 * on the order, the traffic does. PUT THE MOST SELECTIVE PREDICATE FIRST. A range with
 * neither bound matches every row and its column is not read; a range that no int32 can
 * satisfy gives K = 0, or the empty aggregate, without reading any column (the outputs are
 * still written on `stream`). Integer operations only: the result is bitwise the same
 * whatever the grid, the order of the predicates or the alignment of the pointers. Columns
 * that are not all 16-byte aligned are read with dword loads.
 * Both calls are asynchronous on `stream`. d_ws: mq_where_workspace_bytes(n) bytes, 16-byte
 * aligned (positions: one bit per row, a count per 256 rows and the scan's scratch behind
 * the per-block partials). n == 0 gives K = 0, or the empty aggregate, and MQ_OK.
 * MQ_EINVAL, with nothing written: ncols outside 1..8, n >= 2^31, a NULL h_ranges or
 * d_cols, a NULL or not 4-byte aligned column, payload, value column or output with n > 0,
 * a NULL output count or aggregate, a NULL, short or misaligned workspace. */
enum { MQ_WHERE_MAX_COLS = 8 };
typedef struct mq_range { int32_t has_low, low, has_high, high; } mq_range;   /* 16 bytes */
size_t mq_where_workspace_bytes(uint64_t n);          /* needs no device */
int mq_where_positions(const int32_t* const* d_cols /* host array of ncols device pointers */,
                       const mq_range* h_ranges, int ncols, const int32_t* d_payload /* may be NULL */,
                       uint64_t n, int32_t* d_pos_out /* capacity n */, uint64_t* d_count /* device */,
                       void* d_ws, size_t ws_bytes, void* stream);
int mq_where_agg(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols,
                 const int32_t* d_val, uint64_t n, mq_agg* d_out /* device */,
                 void* d_ws, size_t ws_bytes, void* stream);

/* ---- WHERE ... AND k [NOT] IN (SELECT ...): semi and anti join in one pass ----
 * A key set is the subquery's column as a bitmap: one bit per value of its span [lo, hi],
 * bit (uint32)(key - lo) for `key`, in 32-bit words, rounded up to 16 bytes and zeroed (512 MiB
 * at the full int32 span, so the span needs no second representation).
 * build: has_bounds gives the span as {lo, hi}, inclusive (as mq_group_plan's key bounds): a key
 *        outside it fails the build with MQ_EINVAL, everything released and *out = NULL.
 *        Without bounds the span is the column's min and max, one more read of the keys
 *        (mq_reduce). One streaming pass sets the bits (a global atomic OR, skipped when the
 *        bit is seen set already: a column of one hot key does not queue n1 atomics on one
 *        address), a second small kernel counts them: h_info->distinct is COUNT(DISTINCT) of the
 *        column. The call SYNCHRONISES `stream` (the host reads the bounds and the count);
 *        once it returns the handle is immutable and may be probed on any stream of its
 *        device, any number of times, concurrently. n1 == 0 gives the empty set (lo = 0,
 *        hi = -1, no bitmap) and a handle to free. mq_keyset_free: once every probe of the
 *        handle has completed (the caller synchronises); NULL is fine.
 *        MQ_EINVAL: n1 >= 2^31, d_keys NULL or not 4-byte aligned with n1 > 0, lo > hi with
 *        has_bounds, a NULL out. MQ_ENOMEM when the bitmap cannot be allocated.
 * probe: row i matches when every one of the ncols (0 .. MQ_WHERE_MAX_COLS) ranges holds, with
 *        mq_where_positions' semantics exactly, and d_key[i] is in the set; with anti != 0,
 *        when d_key[i] is NOT in the set. A key outside [lo, hi] is not in the set (one
 *        unsigned compare, right at both ends of int32 and for the full span). Outputs,
 *        ordering, payload, the empty aggregate and the workspace (mq_semi_workspace_bytes(n)
 *        bytes, 16-byte aligned) are mq_where_positions' and mq_where_agg's; with ncols == 0
 *        d_cols and h_ranges may be NULL. d_key may be a predicate column or the value column.
 *        The ranges are evaluated first, in the order given; of the key column only the
 *        128-byte lines that still hold a row are requested, the set is looked up for
 *        surviving rows only, and the aggregate's value column follows under the same rule.
 *        With ncols == 0 the key column is the one read whole.
 * path:  MQ_SEMI_LDS: every block copies the bitmap into LDS first and looks up there;
 *        MQ_SEMI_GLOBAL: the bit's word is a cached load (the bitmap stays in L2 and the
 *        Infinity Cache; the columns pass by with non-temporal loads). MQ_SEMI_AUTO takes LDS
 *        for a bitmap of up to mq_semi_auto_path's threshold. Forcing MQ_SEMI_LDS on a
 *        bitmap above 128 KiB is MQ_EINVAL. The result does not depend on the path.
 * Taken on the host, with no launch over the columns: the empty set gives K = 0 / the empty
 * aggregate (anti == 0) or exactly mq_where_positions / mq_where_agg on the ranges (anti != 0;
 * every row when ncols == 0); a range that no int32 satisfies gives K = 0 as before.
 * Both probes are asynchronous on `stream`, which must belong to the key set's device.
 * MQ_EINVAL, with nothing written: ncols outside 0..8, n >= 2^31, a NULL ks, a NULL or not
 * 4-byte aligned column, key, value, payload or output with n > 0, a NULL count or aggregate,
 * a NULL, short or misaligned workspace, a path that is none of the three, a key set of
 * another device. Nothing here has been measured on a device yet: DESIGN.md §3.17. */
typedef struct mq_keyset mq_keyset;
typedef struct mq_keyset_info {
    int32_t  lo, hi;      /* the set's span, inclusive (lo > hi: the empty set) */
    uint64_t distinct;    /* number of different keys = COUNT(DISTINCT) of the column */
    uint64_t bytes;       /* size of the bitmap */
} mq_keyset_info;
int mq_keyset_build(const int32_t* d_keys, uint64_t n1,
                    int has_bounds, int32_t lo, int32_t hi,
                    mq_keyset** out, mq_keyset_info* h_info /* may be NULL */, void* stream);
int mq_keyset_free(mq_keyset* ks);
enum { MQ_SEMI_AUTO = 0, MQ_SEMI_LDS = 1, MQ_SEMI_GLOBAL = 2 };
size_t mq_semi_workspace_bytes(uint64_t n);             /* needs no device */
int mq_semi_auto_path(uint64_t set_bytes);              /* needs no device: MQ_SEMI_LDS or MQ_SEMI_GLOBAL */
int mq_semi_positions(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols /* 0..8 */,
                      const int32_t* d_key, const mq_keyset* ks, int anti, int path,
                      const int32_t* d_payload /* may be NULL */, uint64_t n,
                      int32_t* d_pos_out /* capacity n */, uint64_t* d_count /* device */,
                      void* d_ws, size_t ws_bytes, void* stream);
int mq_semi_agg(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols,
                const int32_t* d_key, const mq_keyset* ks, int anti, int path,
                const int32_t* d_val, uint64_t n, mq_agg* d_out /* device */,
                void* d_ws, size_t ws_bytes, void* stream);

/* ---- GROUP BY an attribute of a joined dimension, in one pass ----
 *   SELECT d.attr, count(*), sum(f.v), min(f.v), max(f.v) FROM f JOIN d ON f.fkey = d.key
 *   WHERE f.c0 IN [..) AND ... GROUP BY d.attr
 * A key map is the dimension (d_keys a primary key, d_attrs its attribute) as a map from key to
 * attribute, in one representation for every span: the key set's bitmap over [lo, hi] (built by
 * mq_keyset_build's code; mq_keymap_keyset returns it as an ordinary key set that the map
 * owns), a rank directory of one uint64_t per 32 keys of the span (low 32 bits the bitmap word,
 * high 32 bits the set bits of all earlier words, an exclusive prefix below 2^31) and the
 * attributes in key order. A lookup is d = (uint32_t)(key - lo) <= hi - lo, one 8-byte load
 * e = dir[d >> 5], a bit test, rank = (e >> 32) + popc((uint32_t)e & ((1u << (d & 31)) - 1)) and
 * one 4-byte load attr_by_rank[rank]. At the full int32 span that is 512 MiB of bitmap plus
 * 1 GiB of directory plus 4 * n1 bytes (mq_keymap_bytes(span, n1), span = hi - lo + 1 up to 2^32).
 * build: the bounds are mq_keyset_build's (given, or one mq_reduce over the keys; a key outside
 *        given bounds is MQ_EINVAL). The keys must be distinct: otherwise MQ_EINVAL,
 *        mq_last_error() names the number of repeated keys, and everything is released. A
 *        prefix pass over the bitmap words' popcounts writes the directory (a fixed grid of
 *        chunks, mq_keymap_geometry: blocks and bitmap words a chunk, no device needed),
 *        k_keymap_place stores every attribute at its key's rank, and one mq_reduce over the
 *        attributes gives attr_lo / attr_hi. SYNCHRONISES `stream`; afterwards the handle is
 *        immutable and may be probed on any stream of its device. n1 == 0 gives the empty map
 *        (lo = 0, hi = -1, attr_lo = INT32_MAX, attr_hi = INT32_MIN) and a handle to free.
 *        MQ_EINVAL otherwise as mq_keyset_build, and for NULL or misaligned attributes.
 * lookup: the materialised N:1 join, SELECT d.attr FROM f JOIN d: for i < k < 2^31, with
 *        key = d_keys[d_pos ? d_pos[i] : i], d_attr_out[i] = the key's attribute, or `missing`
 *        when the key is not in the map; d_hit_out[i] (may be NULL) = 1 or 0. Grid-stride,
 *        asynchronous on `stream`; nothing is written at or past entry k.
 * mq_group_join_plan: with m[i] = every range holds for row i (mq_where_positions' meaning;
 *        ncols == 0: every row, d_cols and h_ranges may then be NULL) and d_fkey[i] is in the
 *        map, the result is exactly mq_group_plan over (attr(d_fkey[m]), d_vals[m]): an inner
 *        join, fact rows without a partner are dropped. *h_rows (may be NULL) = the joined
 *        rows. The handle is an ordinary mq_group with one key: mq_group_write (d_keys_out
 *        receives the attributes) and mq_group_free serve it. Integer operations only: bitwise
 *        the same whatever the path, the grid, the order of the predicates or the alignment.
 *        h_attr_bounds (NULL or a host {lo, hi}, inclusive) constrains the attributes of JOINED
 *        rows only; one outside them is MQ_EINVAL with everything released and is never used
 *        as an address. NULL takes the map's attr_lo / attr_hi and costs no pass over the fact
 *        table. The range picks the path as in mq_group_plan; MQ_GROUP_DENSE forced on a wider
 *        range is MQ_EINVAL.
 * dense: one streaming pass, k_group_join_dense: k_group_where_dense with the lookup between
 *        the key column and the tables. Of d_fkey only the 128-byte lines with a surviving row
 *        are requested; for surviving rows only, the directory entry and then, for hits, the
 *        attribute; of d_vals only the lines that still hold a joined row. The fact columns
 *        pass by with non-temporal loads, directory and attributes with plain cached loads.
 * sort:  mq_semi_positions on the map's key set gives the K joined rows, mq_keymap_lookup
 *        through them their attributes, mq_fetch their values (a buffer the handle owns), then
 *        mq_group_plan's sort path on those.
 * Settled on the host with no launch over the columns: n == 0, a range that no int32 satisfies,
 * the empty map: zero groups and a handle to free. Pointer, ncols (0..8 here), n and path checks
 * are mq_group_where_plan's; a key map of another device is MQ_EINVAL. Synchronises.
 * Not measured on a device yet (tools/bench_group_join.py is the sweep). */
typedef struct mq_keymap mq_keymap;
typedef struct mq_keymap_info {
    int32_t  lo, hi;            /* span of the keys, inclusive (lo > hi: empty map) */
    int32_t  attr_lo, attr_hi;  /* min / max of the attributes (INT32_MAX / INT32_MIN when empty) */
    uint64_t entries;           /* n1 */
    uint64_t bytes;             /* device bytes held: bitmap + directory + attributes */
} mq_keymap_info;
size_t mq_keymap_bytes(uint64_t span, uint64_t n1);      /* needs no device */
/* the directory's prefix pass over a span of `span` keys: blocks launched and bitmap words
 * (32 keys each) in a block's chunk; needs no device, either pointer may be NULL */
void mq_keymap_geometry(uint64_t span, uint32_t* prefix_blocks, uint64_t* prefix_chunk_words);
int mq_keymap_build(const int32_t* d_keys, const int32_t* d_attrs, uint64_t n1,
                    int has_bounds, int32_t lo, int32_t hi,
                    mq_keymap** out, mq_keymap_info* h_info /* may be NULL */, void* stream);
const mq_keyset* mq_keymap_keyset(const mq_keymap* km);  /* the same keys as a §3.17 key set; owned by km */
int mq_keymap_lookup(const mq_keymap* km, const int32_t* d_keys, const int32_t* d_pos /* may be NULL */,
                     uint64_t k, int32_t missing, int32_t* d_attr_out,
                     uint8_t* d_hit_out /* may be NULL */, void* stream);
int mq_keymap_free(mq_keymap* km);
int mq_group_join_plan(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols /* 0..8 */,
                       const int32_t* d_fkey, const mq_keymap* km, const int32_t* d_vals, uint64_t n,
                       const int32_t* h_attr_bounds /* NULL: the map's attr_lo, attr_hi */, int path,
                       mq_group** out, uint64_t* h_groups, int* h_path, uint64_t* h_rows, void* stream);

/* ---- GROUP BY over several joined dimensions, in one pass ----
 *   SELECT d1.a, d2.b, f.k, count(*), sum(f.v), min(f.v), max(f.v)
 *   FROM f JOIN d1 ON f.k1 = d1.key JOIN d2 ON f.k2 = d2.key [JOIN d3 ... only as a filter]
 *   WHERE f.c0 IN [..) AND ... GROUP BY d1.a, d2.b, f.k
 * A term is a fact column and what it means (mq_star_term): with `km`, the column is a foreign
 * key into that key map, the row is kept when the key has a partner, and the partner's attribute
 * is a component of the group tuple; with `ks`, the row is kept when the value is in that key set
 * and the term gives no component (a dimension joined only as a filter); with neither, the value
 * itself is a component (a fact-side group key). Both set is MQ_EINVAL. nkeys = the terms without
 * `ks`, 1..MQ_GROUP_MAX_KEYS.
 * Row i is JOINED when every range holds (mq_where_positions' meaning; ncols == 0: every row,
 * d_cols and h_ranges may then be NULL) and every km / ks term finds d_col[i]. Its tuple is the
 * components of the non-ks terms in the order given, the first most significant.
 * mq_group_star_plan: the result is exactly mq_group_by_plan over the joined rows' tuples and
 *        values: one entry per distinct tuple in ascending lexicographic signed order, uint64_t
 *        count, exact int64_t sum, min and max. Integer operations only: bitwise the same
 *        whatever the path, the grid, the alignment, the order of the ranges, or the place of
 *        the ks terms among the others. *h_rows (may be NULL) = the joined rows. The handle is an
 *        ordinary mq_group: with nkeys == 1 exactly what mq_group_join_plan leaves (mq_group_write
 *        writes the component), with nkeys > 1 what mq_group_by_plan leaves (mq_group_by_write).
 *        Shapes that the older plans could serve are not handed to them.
 * bounds: h_key_bounds is {lo_0, hi_0, ..} per component, inclusive, and constrains JOINED rows
 *        only: a joined row's component outside its own bounds is MQ_EINVAL with everything
 *        released, and is never used as an address (every component is checked by itself, not the
 *        summed code). With NULL, a km component takes the map's attr_lo / attr_hi at no cost,
 *        and a plain component takes one mq_reduce over its WHOLE column: all n rows, joined or
 *        not, so a stray value in a dropped row widens the key space (and may move the plan to
 *        the sort path or past 2^32). Bounds from the caller avoid that pass. P = prod(hi_j -
 *        lo_j + 1) picks the path as in mq_group_by_plan; MQ_GROUP_DENSE forced past
 *        mq_group_dense_slots(), or P > 2^32, is MQ_EINVAL.
 * order: the ranges run first, in the order given, then the terms in the order given. Of each
 *        term's column only the 128-byte lines that still hold a row are requested, and a lookup
 *        is made for surviving rows only: put the most selective filter first, as for
 *        mq_where_positions.
 * dense: one streaming pass, k_group_star_dense: per term the surviving lines of its column
 *        (non-temporal), then the set's bitmap word, or the map's directory entry and for hits the
 *        attribute (plain cached loads, global memory only: there is no LDS form of the lookups);
 *        the tuple code addresses k_group_by_where_dense's per-block LDS tables.
 * sort:  mq_star_positions gives the K joined rows; k_group_star_pack_pos reads every component
 *        through them and writes the codes, mq_fetch gathers the values into a buffer the handle
 *        owns, then mq_group_plan's sort path runs on the codes.
 * Settled on the host with no launch over the columns: n == 0, a range that no int32 satisfies,
 * an empty map or set among the terms: MQ_OK, zero groups and a handle to free.
 * MQ_EINVAL with nothing allocated: nterms outside 1..MQ_STAR_MAX_TERMS, nkeys outside
 * 1..MQ_GROUP_MAX_KEYS (terms that are all ks), km and ks in one term, a map or set of another
 * device; pointer, ncols (0..8 here), n and path rules are mq_group_by_where_plan's. Synchronises.
 * mq_star_positions: mq_semi_positions with the conjunction of all km / ks terms behind the
 *        ranges (a plain term places no condition; nterms 1..MQ_STAR_MAX_TERMS):
 *        d_payload ? d_payload[i] : i of every joined row, ascending i, and their number K in
 *        *d_count. Workspace mq_semi_workspace_bytes(n), 16-byte aligned; asynchronous on
 *        `stream`; nothing is written at or past entry K. k_star_mask probes the global bitmap
 *        (for a km term the map's own key set bitmap, 4-byte words, not the directory); there is
 *        no LDS form. n == 0, an unsatisfiable range or an empty map or set write K = 0.
 * Not measured on a device yet (tools/bench_star.py is the sweep). */
enum { MQ_STAR_MAX_TERMS = 4 };
typedef struct mq_star_term {          /* 24 bytes */
    const int32_t*   d_col;            /* a fact column, n rows */
    const mq_keymap* km;               /* grouped through a dimension: component = attribute of d_col[i] in km */
    const mq_keyset* ks;               /* filter only: row kept when d_col[i] is in ks; no component */
} mq_star_term;                        /* km == ks == NULL: d_col[i] itself is the component; both set: MQ_EINVAL */
int mq_star_positions(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols /* 0..8 */,
                      const mq_star_term* h_terms, int nterms /* 1..4 */,
                      const int32_t* d_payload /* may be NULL */, uint64_t n,
                      int32_t* d_pos_out, uint64_t* d_count /* device */, void* d_ws, size_t ws_bytes, void* stream);
int mq_group_star_plan(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols /* 0..8 */,
                       const mq_star_term* h_terms, int nterms /* 1..4 */,
                       const int32_t* d_vals, uint64_t n,
                       const int32_t* h_key_bounds /* NULL or 2*nkeys host ints */, int path,
                       mq_group** out, uint64_t* h_groups, int* h_path, uint64_t* h_rows, void* stream);

/* ---- Several expression aggregates over a star query's groups, in one pass ----
 *   SELECT d1.a, f.k, count(*), sum(f.x), min(f.x), max(f.x), sum(f.x * f.y), .., sum(f.x - f.z), ..
 *   FROM f JOIN d1 .. WHERE .. GROUP BY d1.a, f.k
 * The joined rows, the tuples, their order, the bounds rules, *h_rows and the shapes settled on the
 * host (n == 0, an unsatisfiable range, an empty map or set) are exactly mq_group_star_plan's with
 * the same ranges, terms and bounds. In place of one value column there are nmeas measures
 * (1..MQ_GROUP_MAX_MEASURES), each a column or a binary expression of two columns (mq_measure).
 * value: for row i, computed EXACTLY in int64 from the int32 operands: a, a + b, a - b or a * b
 *        (|a * b| <= 2^62: all four fit). This is not mq_add / mq_sub's int32 wrap:
 *        INT32_MIN - INT32_MAX is -4294967295.
 * outputs: per group one uint64_t count and, per measure, an int64_t sum, min and max over the
 *        group's joined rows. The sum is taken modulo 2^64 (two's complement; accumulated in
 *        unsigned 64-bit everywhere, so no signed overflow is evaluated) and is therefore bitwise
 *        independent of the order of addition, the path, the grid and the alignment.
 * aliasing: any operand may be the same column as the other operand, a term's or a predicate's.
 * reads: the host collects the DISTINCT operand pointers (at most 8); the dense kernel loads each
 *        once per tile, and of each only the 128-byte lines that still hold a joined row. A
 *        dropped row's operands never reach an aggregate.
 * dense: a slot costs 4 + 24 * nmeas bytes of LDS (u32 count; u64 sum, i64 min, i64 max per
 *        measure). mq_group_measures_dense_slots(nmeas) is the largest power of two whose table
 *        fits the 40 KiB of every dense grouping kernel: 1024, 512, 512, 256 for nmeas 1..4 (0 for
 *        any other nmeas). P = prod(hi_j - lo_j + 1) <= that capacity takes the dense path under
 *        MQ_GROUP_AUTO; MQ_GROUP_DENSE forced past it, or P > 2^32, is MQ_EINVAL.
 *        mq_group_measures_auto_path answers from bounds alone, as mq_group_by_auto_path does.
 *        mq_group_dense_slots() and the single-value plans are unchanged.
 *        k_group_measures_dense: k_group_star_dense's front half, then the operand lines, the
 *        measures (op is uniform over the grid) and LDS atomics (one on the count and a 64-bit add,
 *        min and max per measure), with the wave-uniform run fold; k_measures_fold,
 *        k_measures_rank and k_measures_dense_write serve the wider slot.
 * sort:  mq_star_positions gives the K joined rows, k_group_star_pack_pos their codes,
 *        k_measures_eval_pos one int64 column of K values per measure; mq_index_build sorts the
 *        codes and k_measures_seg_write folds the values through the sorted positions. The handle
 *        owns every buffer and frees them in the order of the stream of the last write.
 * contract: the plan SYNCHRONISES. The write is asynchronous on `stream`, may be repeated (on any
 *        stream of the device), takes NULL for d_keys_out, d_count_out, d_sum_out, d_min_out,
 *        d_max_out or for any entry of the host arrays (nkeys resp. nmeas device pointers), and
 *        writes nothing at or past entry *h_groups. The measure columns must stay valid until the
 *        last write has completed.
 * MQ_EINVAL with *out = NULL, *h_groups = 0, *h_rows = 0 and nothing allocated: everything
 * mq_group_star_plan refuses; nmeas outside 1..4; a NULL h_meas; an op outside the four; with
 * n > 0 a NULL or not 4-byte aligned d_a (or misaligned d_b); d_b NULL for a binary op or non-NULL
 * for MQ_MEAS_COL; reserved != 0. A joined row with a component out of its bounds is MQ_EINVAL with
 * everything released, and is never used as an address.
 * Not measured on a device yet (tools/bench_measures.py is the sweep). */
enum { MQ_GROUP_MAX_MEASURES = 4 };
enum { MQ_MEAS_COL = 0, MQ_MEAS_ADD = 1, MQ_MEAS_SUB = 2, MQ_MEAS_MUL = 3 };
typedef struct mq_measure {            /* 24 bytes */
    const int32_t* d_a;                /* n rows */
    const int32_t* d_b;                /* n rows; must be NULL for MQ_MEAS_COL */
    int32_t op, reserved;              /* MQ_MEAS_*; reserved must be 0 */
} mq_measure;
typedef struct mq_mgroup mq_mgroup;
uint32_t mq_group_measures_dense_slots(int nmeas);      /* needs no device; 0 for nmeas outside 1..4 */
/* needs no device: MQ_GROUP_DENSE or MQ_GROUP_SORT for the bounds' key space (*h_space, may be NULL);
 * MQ_EINVAL for empty bounds, a space past 2^32, nkeys or nmeas outside 1..4 */
int mq_group_measures_auto_path(const int32_t* h_key_bounds, int nkeys, int nmeas, uint64_t* h_space);
int mq_group_measures_plan(const int32_t* const* d_cols, const mq_range* h_ranges, int ncols /* 0..8 */,
                           const mq_star_term* h_terms, int nterms /* 1..4 */,
                           const mq_measure* h_meas, int nmeas /* 1..4 */, uint64_t n,
                           const int32_t* h_key_bounds /* NULL or 2*nkeys host ints */, int path,
                           mq_mgroup** out, uint64_t* h_groups, int* h_path, uint64_t* h_rows, void* stream);
int mq_group_measures_write(mq_mgroup* g, int32_t* const* d_keys_out /* NULL or nkeys ptrs, any NULL */,
                            uint64_t* d_count_out,
                            int64_t* const* d_sum_out, int64_t* const* d_min_out, int64_t* const* d_max_out
                            /* each NULL or a host array of nmeas device pointers, any of them NULL */,
                            void* stream);
int mq_group_measures_free(mq_mgroup* g);

/* ---- COUNT(DISTINCT v) per group under a WHERE ----
 *   SELECT k0, .., count(DISTINCT v) FROM t WHERE c0 IN [..) AND .. GROUP BY k0, ..
 * With m[i] = every range holds for row i (mq_where_positions' meaning; ncols == 0: every row,
 * d_cols and h_ranges may be NULL): one entry per distinct key tuple (nkeys in 1..MQ_GROUP_MAX_KEYS)
 * that has a matching row, in ascending lexicographic signed order (mq_group_by_where_plan's order:
 * the two operators' key outputs are identical), each with the number of different values of d_vals
 * among the tuple's matching rows, as u64. Integer compares and bit sets only: the result is
 * bitwise the same on every path, grid, alignment, predicate order and block finishing order.
 * With P = prod(hi_j - lo_j + 1) of the key bounds, W = vhi - vlo + 1 of the value bounds and
 * R = ceil(W / 32), a group's values are one row of R 32-bit words of a bitmap of P rows (the
 * padding bits are never set and never counted):
 * lds    (4 P R <= mq_group_distinct_lds_bytes()): one streaming pass in k_group_by_where_dense's
 *        shape (the predicates, then the key and value lines that hold a survivor); a survivor
 *        sets bit code * 32 R + (v - vlo) in a per-block LDS bitmap, which the block ORs into the
 *        global bitmap at the end of its chunk.
 * bitmap (4 P R <= mq_group_distinct_bitmap_bytes(), 512 MiB, the key set's cap): the same pass,
 *        marking the zeroed global bitmap with mq_keyset_build's load-then-atomic-OR.
 *        After either: one popcount per row, and the non-empty rows compacted in code order
 *        (mq_select_positions with low = 1 over the counts, then mq_fetch).
 * sort   (P <= 2^32, any W): mq_where_positions (skipped with ncols == 0), the packed codes of
 *        mq_group_by_where_plan's sort path, the values gathered, mq_index_build by value and
 *        then, stable, by code, so that the rows are in (code, value) order; a group's count is
 *        the number of rows in its run whose code or value differs from the row before.
 * MQ_GDISTINCT_AUTO takes the first path whose size rule holds; the rule is by size only, and
 * nobody has measured where bitmap loses to sort. A forced path whose rule does not hold is
 * MQ_EINVAL. Not measured on a device yet: DESIGN.md §3.22.
 * Bounds (inclusive; h_key_bounds {lo_0, hi_0, ..}, h_val_bounds {vlo, vhi}) constrain MATCHING
 * rows only: a key or value of a row that fails a predicate is never an error and never an
 * address. Every key component and the value of a matching row is checked against its own
 * bounds; a violation is MQ_EINVAL with everything released. NULL key bounds cost one more pass
 * (k_group_by_where_bounds; one mq_reduce per key column with ncols == 0), NULL value bounds one
 * mq_where_agg over the value column (one mq_reduce with ncols == 0).
 * The plan SYNCHRONISES and finishes the whole computation: the handle owns only the groups'
 * codes and counts, and no input needs to outlive the plan. The write is asynchronous and
 * repeatable, skips NULL outputs and writes nothing at or past *h_groups entries. n == 0, a range
 * that no int32 satisfies or no matching row give MQ_OK, zero groups and a handle to free (h_info:
 * the forced path, or MQ_GDISTINCT_LDS, and zeros).
 * MQ_EINVAL, with *out = NULL, *h_groups = 0 and nothing allocated: ncols outside 0..8, nkeys
 * outside 1..4, n >= 2^31, a NULL or not 4-byte aligned pointer with n > 0, a NULL out or
 * h_groups, a path outside the four, and of given bounds with n > 0 lo > hi, P > 2^32 or a
 * forced path whose rule does not hold. */
enum { MQ_GDISTINCT_AUTO = 0, MQ_GDISTINCT_LDS = 1, MQ_GDISTINCT_BITMAP = 2, MQ_GDISTINCT_SORT = 3 };
typedef struct mq_gdistinct mq_gdistinct;
typedef struct mq_gdistinct_info {
    int      path;         /* the path taken */
    uint64_t space;        /* P = prod(hi_j - lo_j + 1) of the key bounds used */
    uint64_t span;         /* W = vhi - vlo + 1 of the value bounds used, up to 2^32 */
    uint64_t bitmap_bytes; /* 4 * P * R, R = ceil(W / 32); 0 on the sort path */
    uint64_t rows;         /* rows that passed the predicates */
    uint64_t pairs;        /* distinct (tuple, value) pairs = the sum of the distinct counts */
} mq_gdistinct_info;
uint64_t mq_group_distinct_lds_bytes(void);     /* constants; need no device */
uint64_t mq_group_distinct_bitmap_bytes(void);  /* 512 MiB, the key set's cap */
/* needs no device: the path AUTO takes, or MQ_EINVAL (nkeys outside 1..4, a NULL pointer, a lo > hi,
 * P > 2^32); *h_bitmap_bytes (may be NULL) = 4 * P * R, UINT64_MAX when P > 2^32 */
int mq_group_distinct_auto_path(const int32_t* h_key_bounds, int nkeys, const int32_t* h_val_bounds,
                                uint64_t* h_bitmap_bytes /* may be NULL; saturated */);
int mq_group_distinct_plan(const int32_t* const* d_cols, const struct mq_range* h_ranges, int ncols /* 0..8 */,
                           const int32_t* const* d_keys, int nkeys /* 1..4 */, const int32_t* d_vals, uint64_t n,
                           const int32_t* h_key_bounds /* NULL or 2*nkeys */, const int32_t* h_val_bounds /* NULL or {lo,hi} */,
                           int path, mq_gdistinct** out, uint64_t* h_groups, mq_gdistinct_info* h_info /* may be NULL */,
                           void* stream);
int mq_group_distinct_write(mq_gdistinct* g, int32_t* const* d_keys_out /* NULL, or nkeys ptrs, any NULL */,
                            uint64_t* d_distinct_out /* may be NULL */, void* stream);
int mq_group_distinct_free(mq_gdistinct* g);

/* ---- S5 fetch_column: d_out[i] = d_col[d_pos[i]] ---- */
int mq_fetch(const int32_t* d_col, const int32_t* d_pos, uint64_t k, int32_t* d_out, void* stream);
/* the same from a row shard holding rows [row_base, row_base + rows) of the column:
 * d_out[i] = d_col[d_pos[i] - row_base] (every position must lie in the shard) */
int mq_fetch_at(const int32_t* d_col, int32_t row_base, const int32_t* d_pos, uint64_t k, int32_t* d_out,
                void* stream);

/* ---- S7/S8/S9 over a values vector (sum/avg/min/max of a Result) ---- */
int mq_reduce(const int32_t* d_vals, uint64_t n, mq_agg* d_out, void* d_ws, size_t ws_bytes,
              void* stream);

/* ---- P1 print (query.c:245-304): int32 values as decimal text ----
 * Writes "%d" of every value, joined by "\n" (no trailing separator, no NUL),
 * into d_out (capacity >= 12 * n bytes); *h_len receives the byte count. The
 * call synchronises the stream. d_ws: >= mq_format_workspace_bytes(n). */
size_t mq_format_workspace_bytes(uint64_t n);
int mq_format_int32(const int32_t* d_vals, uint64_t n, char* d_out, uint64_t* h_len, void* d_ws,
                    size_t ws_bytes, void* stream);

/* A table as CSV text, the way the reference's generators write the load files
 * (value of column 0, ',' ... column ncols-1, '\n' per row; "%d" each). d_cols: host
 * array of ncols device pointers; d_out capacity >= rows * ncols * 12 bytes; *h_len
 * receives the byte count. Synchronises the stream. (Bench/test data for the load
 * path; the reference loads such files with load_db.) */
size_t mq_format_csv_workspace_bytes(uint64_t rows, int ncols);
int mq_format_csv_int32(const int32_t* const* d_cols, int ncols, uint64_t rows, char* d_out,
                        uint64_t* h_len, void* d_ws, size_t ws_bytes, void* stream);

/* ---- load path: load_db's data loop (db_manager.c:304-318) + insert_row (:164-199) ----
 * d_text: n bytes of CSV data lines in HBM (the header line already consumed; the
 * header is what fgets returns first, <= 1023 bytes through '\n'). Rows are the
 * reference's fgets(line, 1024) pieces: through the next '\n', at most 1023 bytes.
 * Each row's first ncols ','-separated tokens go through atoi; a token missing from
 * a row keeps the previous row's value (0 before the first row); extra tokens are
 * ignored. Two steps on one workspace (mq_csv_workspace_bytes(n, ncols)):
 * count: *h_rows = rows (synchronous);
 * parse: d_cols[j] (host array of ncols device pointers, capacity >= rows) receive
 *        column j; d_minmax (device, 2*ncols int32) min/max per column (INT32_MAX /
 *        INT32_MIN when rows == 0), as insert_row folds them. ncols <= 1024. */
size_t mq_csv_workspace_bytes(uint64_t n, int ncols);
int mq_csv_count_rows(const char* d_text, uint64_t n, int ncols, uint64_t* h_rows, void* d_ws,
                      size_t ws_bytes, void* stream);
int mq_csv_parse_int32(const char* d_text, uint64_t n, int ncols, int32_t* const* d_cols,
                       uint64_t rows, int32_t* d_minmax, void* d_ws, size_t ws_bytes, void* stream);

/* ---- S10 add / sub (int32, two's-complement wrap) ---- */
int mq_add(const int32_t* d_a, const int32_t* d_b, uint64_t n, int32_t* d_out, void* stream);
int mq_sub(const int32_t* d_a, const int32_t* d_b, uint64_t n, int32_t* d_out, void* stream);

/* ---- S11 shared_select: q range predicates [lows[j], highs[j]) over one column ----
 * h_lows/h_highs: q host int32 bounds, used as given (has_low/has_high are ignored
 * there, query.c:472-479). d_pos_out[j] (host array of q device pointers, each of
 * capacity n) receives query j's ascending positions; d_counts[j] (device) its K_j.
 * q >= 2 reads the column twice in total (count pass + write pass), any q <= 256. */
size_t mq_shared_select_workspace_bytes(uint64_t n, int q);
int mq_shared_select(const int32_t* d_col, uint64_t n, const int32_t* h_lows,
                     const int32_t* h_highs, int q, int32_t* const* d_pos_out,
                     uint64_t* d_counts, void* d_ws, size_t ws_bytes, void* stream);
/* The same in two steps, so outputs can be sized exactly (q <= 256):
 * count: one pass, *h_counts[j] = K_j (host, synchronous); the workspace keeps the
 *        offsets for the next step;
 * write: the second pass into d_pos_out[j] (capacity K_j each), on the workspace
 *        of the immediately preceding count call of this thread. */
int mq_shared_select_count(const int32_t* d_col, uint64_t n, const int32_t* h_lows,
                           const int32_t* h_highs, int q, uint64_t* h_counts, void* d_ws,
                           size_t ws_bytes, void* stream);
int mq_shared_select_write(void* d_ws, int32_t* const* d_pos_out, void* stream);
/* count over a row shard whose rows number from row_base (the write then emits
 * row_base + i), as mq_select_positions_at */
int mq_shared_select_count_at(const int32_t* d_col, uint64_t n, int32_t row_base, const int32_t* h_lows,
                              const int32_t* h_highs, int q, uint64_t* h_counts, void* d_ws,
                              size_t ws_bytes, void* stream);

/* ---- J1 hash_join as three steps on a handle (lets the caller size the output) ----
 * build: table over (c1, p1); c1 and p1 must stay valid until mq_join_free (a unique
 *   build of 2^20 rows and more keeps only its window partition, and one whose probe
 *   meets a duplicate key is built again from them).
 * probe: per-probe match counts + output offsets for keys c2; *h_m = M. c2 is read
 *   only inside the call (a partitioned probe leaves its last inverse pass to the write,
 *   which reads the places that pass recorded, not the keys: DESIGN.md §3.3 round 6).
 * write: the M pairs (out1 = build positions, out2 = probe positions p2). */
typedef struct mq_join mq_join;
int mq_join_build(const int32_t* d_c1, const int32_t* d_p1, uint64_t n1, mq_join** out,
                  void* stream);
int mq_join_probe(mq_join* join, const int32_t* d_c2, uint64_t n2, uint64_t* h_m, void* stream);
int mq_join_write(mq_join* join, const int32_t* d_p2, int32_t* d_out1, int32_t* d_out2,
                  void* stream);
int mq_join_free(mq_join* join);
/* Per probe row of the last mq_join_probe, its number of pairs (d_cnt: n2 u32).
 * mq_join_write also accepts d_p2 = d_out2 = NULL: build positions only. */
int mq_join_counts(mq_join* join, uint32_t* d_cnt, void* stream);

/* ---- key-partitioned hash join over G devices ----
 * The device pieces; mq_shard_join (mq_query.h) runs them over the row-shard workers,
 * analytical-database_amd/dist.py one process per GPU.
 * mq_pjoin_bucket: the bucket (0..G-1) of a key, as the partition kernels compute it.
 * mq_pjoin_partition: stable split of n rows into G buckets by key: d_keys_out (and
 *   d_pay_out with d_pay, and d_inv[r] = row r's new index, when not NULL) hold bucket
 *   0's rows in row order, then bucket 1's, ...; h_counts[b] (host, G entries) their
 *   numbers. Synchronous. G <= 64, n < 2^32.
 * mq_pjoin_place: a probe shard's output from its partitioned counts d_cntp (n u32) and
 *   pairs d_out1p (m build positions, partitioned order): row r's pairs go to the offset
 *   of the rows before it, out2 = d_p2[r]. Asynchronous on stream (its temporaries are
 *   freed stream-ordered). */
uint32_t mq_pjoin_bucket(int32_t key, int G);
int mq_pjoin_partition(const int32_t* d_keys, const int32_t* d_pay, uint64_t n, int G, int32_t* d_keys_out,
                       int32_t* d_pay_out, uint32_t* d_inv, uint64_t* h_counts, void* stream);
int mq_pjoin_place(const uint32_t* d_cntp, const int32_t* d_out1p, const uint32_t* d_inv, const int32_t* d_p2,
                   uint64_t n, uint64_t m, int32_t* d_out1, int32_t* d_out2, void* stream);
/* Device-to-device copy between (or within) devices on stream (the destination's). */
int mq_memcpy_peer(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, void* stream);
/* Let the current device read and write peer's memory directly (a no-op where the
 * platform cannot; peer copies still work then). */
int mq_enable_peer(int peer);

/* ---- J1 hash_join in one call: build on (c1,p1) (n1 rows), probe with (c2,p2) (n2 rows) ----
 * Output pairs (out1[m], out2[m]) = (build position, probe position) in
 * probe-major, build-insertion order (query.c:652-696). *h_m receives M.
 * Returns MQ_ECAP (with *h_m = M) when M > cap. Allocates its own scratch. */
int mq_hash_join(const int32_t* d_c1, const int32_t* d_p1, uint64_t n1, const int32_t* d_c2,
                 const int32_t* d_p2, uint64_t n2, int32_t* d_out1, int32_t* d_out2,
                 uint64_t cap, uint64_t* h_m, void* stream);

#ifdef __cplusplus
}
#endif
#endif
