/*
 * mq_query.h — libmq's drop-in for the reference's operator API.
 *
 * libmq exports exactly the symbols of siyaoL1/Analytical-Database
 * src/include/query.h:20-50, with identical C signatures and struct layouts, so
 * the reference's server.o parse.o client_context.o db_manager.o index.o utils.o
 * link against libmq.so in place of query.o multimap.o (src/Makefile:62).
 * Each entry point below cites the reference function it replaces.
 *
 * The types are re-declared here layout-for-layout from
 * src/include/cs165_api.h:58-132,152-206 and src/include/db_manager.h:95-108;
 * mq_query.c pins every size and offset with _Static_assert (x86-64 SysV).
 * The reference's own headers stay authoritative for its translation units;
 * this header is what libmq itself is compiled against.
 *
 * Ownership (reference contract, client_context.c:31-90, server.c:432):
 * every returned Result / Result** and every payload is malloc'd host memory
 * that the caller frees with free(). Inputs are borrowed.
 * Device residency: a Column's rows are uploaded to HBM on first use and kept
 * while a write guard shows them unchanged; Results produced by libmq keep a
 * device shadow on the same terms (see "residency control" below).
 * Threads: one caller at a time. The residency tables, the write guards and the
 * shard configuration have no lock (the reference's server is one thread); the
 * row-shard workers behind these entry points are libmq's own threads. Callers
 * that want several threads inside libmq use mq_device.h (its "Threads" paragraph).
 */
#ifndef MQ_QUERY_H
#define MQ_QUERY_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- reference ABI types (cs165_api.h) ---- */
#define MQ_MAX_SIZE_NAME 64
#define MQ_HANDLE_MAX_SIZE 64

typedef enum DataType { INT, LONG, FLOAT, DOUBLE } DataType;          /* cs165_api.h:58-63 */

typedef struct ColumnIndex {                                          /* cs165_api.h:65-68 */
    int* values;
    size_t* positions;
} ColumnIndex;

struct Node;       /* btree node, opaque here (btree.h) */
struct Histogram;  /* opaque here (cs165_api.h:71-75) */

typedef struct Column {                                               /* cs165_api.h:77-92 */
    char name[MQ_MAX_SIZE_NAME];
    int* data;
    int fd;
    size_t row_count;
    bool sorted;
    bool clustered;
    bool has_index;
    ColumnIndex* index;
    struct Node* btree_node;
    struct Histogram* histogram;
    int max;
    int min;
} Column;

typedef enum StatusCode { OK, ERROR } StatusCode;                    /* cs165_api.h:152-157 */

typedef struct Status {                                               /* cs165_api.h:160-163 */
    StatusCode code;
    char* error_message;
} Status;

typedef struct Result {                                               /* cs165_api.h:179-183 */
    size_t num_tuples;
    DataType data_type;
    void* payload;
} Result;

typedef enum GeneralizedColumnType { RESULT, COLUMN } GeneralizedColumnType;  /* cs165_api.h:188-191 */

typedef union GeneralizedColumnPointer {                              /* cs165_api.h:195-198 */
    Result* result;
    Column* column;
} GeneralizedColumnPointer;

typedef struct GeneralizedColumn {                                    /* cs165_api.h:203-206 */
    GeneralizedColumnType column_type;
    GeneralizedColumnPointer column_pointer;
} GeneralizedColumn;

typedef struct Table {                                                /* cs165_api.h:110-116 */
    char name[MQ_MAX_SIZE_NAME];
    Column* columns;
    size_t col_count;
    size_t row_count;
    size_t table_length;
} Table;

typedef struct Db {                                                   /* cs165_api.h:127-132 */
    char name[MQ_MAX_SIZE_NAME];
    Table* tables;
    size_t tables_size;
    size_t tables_capacity;
} Db;

/* db_manager.h:95-108; only low/high/column are read by libmq (shared_select). */
typedef struct SelectOperator {
    int select_type;            /* SelectType enum */
    char handle[MQ_HANDLE_MAX_SIZE];
    int low;
    int high;
    int has_low;
    int has_high;
    void* db;
    void* table;
    Column* column;
    Result* col_result;
    Result* pos_result;
    void* comparator;
} SelectOperator;

/* ---- the reference operator API (query.h:20-50) ---- */
Result* select_result(Result* column, Result* position, int* low_pointer, int* high_pointer,
                      Status* ret_status);                          /* query.c:38-86   */
Result* select_column(Column* column, int* low, int* high, Status* ret_status); /* :203-220 */
Result* fetch_column(Column* column, Result* position_result, Status* ret_status); /* :223-243 */
char* print(Result** result, int result_num, Status* ret_status);  /* query.c:245-304 */
Result* average(Result* column, Status* ret_status);                /* query.c:306-323 */
Result* sum(GeneralizedColumn* column, Status* ret_status);          /* query.c:325-354 */
Result* add(Result* column_one, Result* column_two, Status* ret_status);   /* :356-372 */
Result* sub(Result* column_one, Result* column_two, Status* ret_status);   /* :374-390 */
Result* min(Result* column, Status* ret_status);                    /* query.c:392-415 */
Result* max(Result* column, Status* ret_status);                    /* query.c:417-437 */
Result** shared_select(SelectOperator* operators, int query_count, Column* column,
                       Status* ret_status);                         /* query.c:496-583 */
Result** nested_loop_join(Result* column_one, Result* position_one, Result* column_two,
                          Result* position_two, Status* ret_status); /* query.c:585-650 */
Result** hash_join(Result* column_one, Result* position_one, Result* column_two,
                   Result* position_two, Status* ret_status);       /* query.c:652-696 */
void log_result(Result* result);                                    /* query.c:26-36   */
/* also global (undeclared in query.h) in the reference: */
Result* select_column_scan(Column* column, int* low_pointer, int* high_pointer,
                           Status* ret_status);                     /* query.c:92-137  */
Result* select_column_sorted_index(Column* column, int low, int high,
                                   Status* ret_status);             /* query.c:165-198 */
/* index.c:180-185 — exported weak so the reference's index.o definition wins. */
bool should_use_index(Column* column, int low, int high);

/* ---- J4: hashset.h (src/include/hashset.h:7-24) ----
 * hashset.c is not linked into the reference server and has no caller
 * (src/Makefile:62); libmq exports its API so that code
 * written against hashset.h links, with the reference's semantics: `size` int32
 * slots, 0 = empty (0 is never a member), linear probing from hash(key, size).
 * Defined where the reference leaves undefined behaviour: the slots start zeroed
 * (create_hashset mallocs them uninitialised, hashset.c:13), a negative key's probe
 * starts at the wrapped remainder (the reference indexes out of bounds), a full
 * table stops after one lap (it loops forever), and get_hashset_elements returns a
 * buffer sized for its elements (hashset.c:49 allocates 16 bytes). Its element
 * listing runs on the GPU for tables of >= 32768 slots (MQ_HASHSET_GPU_MIN);
 * mq_hashset_lookup (mq_device.h) is the batched device lookup. */
typedef struct hashset {                                              /* hashset.h:7-10 */
    int* keys;
    int size;
} hashset;
int hash(int key, int size);                       /* multimap.c:60-63, exported weak */
hashset* create_hashset(int size);                 /* hashset.c:11-16 */
void free_hashset(hashset* set);                   /* hashset.c:19-22 */
void insert_hashset(hashset* set, int key);        /* hashset.c:25-32 */
bool lookup_hashset(hashset* set, int key);        /* hashset.c:35-45 */
Result* get_hashset_elements(hashset* set);        /* hashset.c:48-65 */
/* Bulk inserts (not in hashset.h): set->keys afterwards holds exactly what
 * `for i in 0..n-1: insert_hashset(set, keys[i])` leaves. From MQ_HASHSET_GPU_MIN
 * keys on (default 32768) and with a device the table is built in HBM
 * (mq_hashset_insert, mq_device.h): table up, build, table down; below that, or
 * without a device, it is that host loop. mq_hashset_insert_result takes the keys of
 * an INT Result (a fetch_column's output, say) from its HBM shadow when one is
 * resident, so they are not uploaded again. Both return 0 or a negative MQ_E* code
 * (MQ_EINVAL for a NULL set, keys or a Result that is not INT); after a device failure
 * set->keys is unchanged and mq_last_error() has the text. */
int mq_hashset_insert_many(hashset* set, const int* keys, size_t n);
int mq_hashset_insert_result(hashset* set, const Result* keys);

/* ---- the load path (db_manager.h:254) ----
 * load_db (db_manager.c:240-322 with insert_row :164-199): same header check
 * (db name, table name), same rows, values, min/max and table_length growth, with
 * the data lines parsed on the GPU (mq_csv_parse_int32). Capacity grows through
 * the server's own save_data / start_data (db_manager.c:430,736), which libmq
 * references weakly: without them (no server linked) a load that must grow the
 * table fails with ERROR. The loaded columns stay resident in HBM for the queries
 * that follow. To use it, the server links this definition instead of
 * db_manager.o's. */
void load_db(Db* db, const char* path, Status* ret_status);

/* ---- the index build (index.c:152-178 build_index, db_manager.h:282) ----
 * For every column with has_index: the sorted copy and its positions on the GPU
 * (mq_index_build), then, as the reference does, clustered: index->positions left
 * 0..n-1 and every other column of the table reordered by the sort permutation;
 * unclustered: index->positions = the permutation plus the 100-bin histogram. The
 * index arrays, histogram and reordered rows are host memory as in the reference
 * (malloc'd / the mmap'd column data); their HBM copies stay resident. Equal values
 * come out in ascending row order (the reference's quicksort orders them its own
 * way). Used like load_db: the server links this definition
 * instead of index.o's. */
void build_index(Db* db);

/* ---- row deletes and updates (the workload generator's milestone 5) ----
 * The DSL of the reference's tests 38-43: relational_delete(db1.tbl5,d1) and
 * relational_update(db1.tbl5.col1,u1,-10). The reference declares no such functions and
 * its parser has no branch for the commands (parse.c:876-960; its server crashes on
 * those tests), so nothing clashes at link time and the semantics are the
 * generator's pandas statements (milestone5.py:127-142, 186-202). Argument order as in
 * the DSL, Status as insert_row. `positions` is an INT Result of row ids, in any order,
 * repeats allowed (a select_column's output); its HBM shadow is used when resident.
 * Both work on the columns' resident copies and leave them resident,
 * so the next operator uploads nothing. Without a device, or with a row id outside the
 * table, they set ERROR and change nothing. A copy attached with mq_column_attach is
 * detached first (the caller's buffer is never written); a column held as row shards
 * drops its shards and is split again on next use.
 * relational_delete: the listed rows leave every column of the table (each column's
 *   row_count must equal table->row_count), the survivors keep their order.
 *   column->data holds the surviving rows, table->row_count and every column's
 *   row_count drop by the number of distinct ids; table_length and the host rows
 *   beyond the new count are left alone, and so are min / max (the reference only ever
 *   widens them, db_manager.c:193-194; they stay valid bounds). Every built index of
 *   the table keeps its entries of surviving rows, in their order, renumbered, in the
 *   same host arrays (the first row_count entries); an unclustered column's histogram
 *   counts are recomputed (bin_size and values[] stay). An empty Result changes nothing.
 * relational_update: column->data[id] = value for every listed id; max / min widen as
 *   insert_row's do; an unclustered index on the column is freed and built again as
 *   build_index builds it. A column with `clustered` set answers ERROR: the reference's
 *   clustered build sorts the index and reorders every OTHER column but leaves this
 *   column's own rows as loaded (index.c:128-133; SURVEY.md §4, FAIL 25), so no row of
 *   it corresponds to a row of the table. The other columns of such a table update
 *   normally. */
void relational_delete(Table* table, Result* positions, Status* ret_status);
void relational_update(Column* column, Result* positions, int value, Status* ret_status);

/* ---- batched row inserts (the workload generator's milestone 5) ----
 * The DSL's relational_insert(db1.tbl5,-1,-11,-111,-1111). The reference declares no
 * function of this name (it is a parser string only, parse.c:885, which calls insert_row,
 * db_manager.c:164-199); libmq does not export insert_row, the server's db_manager.o
 * defines it. `rows` holds nrows x table->col_count ints, row-major: nrows consecutive
 * insert_row rows in the order they would have been issued. `db` is used only when the
 * table must grow and may be NULL otherwise. The operator works on the columns' resident
 * copies and leaves them resident and trusted, so the next operator
 * uploads nothing; a column that was not resident is uploaded once first. Attached copies
 * are detached first and never written; row shards are dropped and split again on next
 * use. nrows == 0 changes nothing.
 * A table without a built clustered index: the rows are appended as insert_row appends
 *   them: host rows [n, n + nrows) of every column, row_count of the table and of every
 *   column, max / min widened (db_manager.c:193-194). The resident copy is extended on the
 *   device from the old copy and an upload of the new values only.
 * A table with a built clustered index on column c stays sorted on it: row r's key is
 *   c->index->values[r], a new row's key its value for c, and the result is the stable
 *   sort by key of the old rows followed by the new ones (a new row lands after every old
 *   row with key <= its own; equal new keys keep batch order). Every column (c's own data
 *   included) and index->values are interleaved that way and written back to the host;
 *   index->positions stays 0..n+nrows-1.
 * Every built unclustered sorted index of the table has the new (value, row) entries
 *   merged in, each after every entry of equal or smaller value, equal new values in batch
 *   order; on a clustered table the old positions are renumbered to the rows' new slots
 *   first. index->values / positions are freed and replaced by malloc'd arrays of the new
 *   length, and the histogram is rebuilt as build_index builds it, from the widened
 *   min / max. A column with has_index whose index was never built gets its rows only.
 * ERROR (a "libmq:" line on stderr, nothing changed): no device, NULL table or rows, more
 *   than 1024 columns, row_count + nrows >= 2^31, a column whose row_count differs from
 *   the table's, a device failure, or row_count + nrows > table_length while the server's
 *   save_data / start_data are not linked or db is NULL. With them the capacity grows as
 *   load_db grows it: one remap to the first table_length * 2^j that fits. */
void relational_insert(Db* db, Table* table, const int* rows, size_t nrows, Status* ret_status);

/* ---- grouped aggregates (not in the reference) ----
 * group_aggregate: count, sum, min and max of `values` per distinct value of `keys`
 * (mq_group_plan / mq_group_write in mq_device.h). Each argument is a
 * COLUMN or an INT RESULT (a fetch_column's output, say), as sum takes them; the two must
 * be equally long and may be the same object. Returns a malloc'd array of five Result*,
 * each with one tuple per distinct key, in ascending key order, and a malloc'd payload the
 * caller frees (the hash_join contract): [0] the keys (INT), [1] the row counts (LONG),
 * [2] the exact sums (LONG), [3] the minima (INT), [4] the maxima (INT). No rows give five
 * empty Results and OK. The INT payloads keep an HBM shadow as every INT Result does. The
 * operator runs on the calling device: a column held as row shards drops them and is split
 * again on next use. A Column's min / max are not taken for key bounds (not every caller
 * that builds a Column maintains them); the keys are read once more for them. ERROR and
 * NULL (a "libmq:" line on stderr): no device, an argument that is neither a Column nor an
 * INT Result, different lengths, 2^31 rows or more, a device failure. */
Result** group_aggregate(GeneralizedColumn* keys, GeneralizedColumn* values, Status* ret_status);

/* ---- ORDER BY ... LIMIT k (not in the reference) ----
 * top_k: the m = min(k, rows) smallest (descending: largest) entries of `values`, in order,
 * with the rows they sit in (mq_topk in mq_device.h). `values` is a COLUMN
 * or an INT RESULT, as sum and group_aggregate take them; `positions` is NULL or an INT
 * Result of the same length, the (column, position) pair select_result takes. Returns a
 * malloc'd array of two Result* with malloc'd payloads the caller frees (the hash_join
 * contract): [0] the m values (INT), ascending, or descending when `descending`; [1] per
 * value its entry of `positions`, or its row id when positions is NULL (INT). Equal values
 * come in ascending input order in both directions, so the result is the first m entries of
 * a stable sort. k == 0 or no rows give two empty Results and OK. Both payloads keep an HBM
 * shadow as every INT Result does; resident copies and shadows of the inputs are used as
 * the other operators use them. The operator runs on the calling device: a column held as
 * row shards drops them and is split again on next use. ERROR and NULL (a "libmq:" line on
 * stderr): no device, an argument of the wrong kind, different lengths, 2^31 rows or more,
 * a device failure. */
Result** top_k(GeneralizedColumn* values, Result* positions, size_t k, bool descending, Status* ret_status);

/* ---- WHERE a IN [..) AND b IN [..) ... (not in the reference) ----
 * A conjunction of 1 to 8 range predicates in one operator (DESIGN.md §3.13;
 * mq_where_positions / mq_where_agg in mq_device.h). The reference's DSL spells it as the
 * chain select_column -> fetch_column -> select_result -> fetch_column -> ...; these return
 * what that chain returns without materialising its intermediates. Each entry of `columns`,
 * and `values`, is a COLUMN or an INT RESULT, as sum and top_k take them; all must be equally
 * long. lows[c] and highs[c] are NULL or point to the bound of columns[c], as select_column's
 * `int* low, int* high`: row i matches when low <= columns[c][i] < high holds for every c.
 * The predicates are evaluated in the order given: put the most selective one first (the
 * answer does not depend on the order, the memory traffic does).
 * select_where: a malloc'd INT Result of the K matching row positions in ascending order,
 *   or, with `positions` (an INT Result as long as the columns), of its entries at those
 *   rows. The payload is obtained, downloaded and shadowed in HBM as select_result's is.
 * aggregate_where: a malloc'd array of four one-tuple Results with malloc'd payloads the
 *   caller frees: [0] the count of matching rows (LONG), [1] the sum of `values` over them
 *   (LONG), [2] their min (INT; INT32_MAX without a match), [3] their max (INT; INT32_MIN).
 *   `values` may be one of the predicate columns.
 * Resident copies and shadows of the inputs are used as the other operators use them. The
 * operator runs on the calling device: a column held as row shards drops them and is split
 * again on next use. ERROR and NULL (a "libmq:" line on stderr): no device, ncols outside
 * 1..8, an argument of the wrong kind, different lengths, 2^31 rows or more, a device
 * failure. */
Result* select_where(GeneralizedColumn** columns, int** lows, int** highs, int ncols,
                     Result* positions /* NULL or INT, same length */, Status* ret_status);
Result** aggregate_where(GeneralizedColumn** columns, int** lows, int** highs, int ncols,
                         GeneralizedColumn* values, Status* ret_status);

/* ---- WHERE ... AND k [NOT] IN (SELECT ...) (not in the reference) ----
 * select_where / aggregate_where with a semi join (anti: an anti join, NOT IN / NOT EXISTS)
 * behind the ranges, in one pass (mq_keyset_build, mq_semi_positions and
 * mq_semi_agg in mq_device.h): row i matches when every range holds and keys[i] is (anti: is
 * not) among the values of `set_keys`. Today's spelling is hash_join's build, probe and
 * per-row counts followed by a select over the counts; an anti join has none.
 * `columns`, `lows`, `highs`, `positions` and `values` are select_where's and
 * aggregate_where's; ncols is 0..8, and with ncols == 0 the first three may be NULL (the IN
 * predicate alone). `keys` is a COLUMN or an INT RESULT as long as the columns; it may be one
 * of them, or `values`. `set_keys` is a COLUMN or an INT RESULT of any length below 2^31, the
 * subquery's output, for instance a select_where or fetch_column Result; duplicates are fine
 * and an empty one is the empty set (semi: no row; anti: the ranges alone).
 * The return values have select_where's and aggregate_where's shapes and ownership. The key
 * set (one bit per value between the smallest and the largest set key, up to 512 MiB) is
 * built per call and freed before returning. Resident copies and shadows of the inputs are
 * used as the other operators use them. The operator runs on the calling device: a column
 * held as row shards drops them and is split again on next use. ERROR and NULL (a "libmq:"
 * line on stderr): no device, ncols outside 0..8, an argument of the wrong kind, different
 * lengths, 2^31 rows or more, a device failure. */
Result* select_where_in(GeneralizedColumn** columns, int** lows, int** highs, int ncols /* 0..8 */,
                        GeneralizedColumn* keys, GeneralizedColumn* set_keys, bool anti,
                        Result* positions /* NULL or INT, same length */, Status* ret_status);
Result** aggregate_where_in(GeneralizedColumn** columns, int** lows, int** highs, int ncols,
                            GeneralizedColumn* keys, GeneralizedColumn* set_keys, bool anti,
                            GeneralizedColumn* values, Status* ret_status);

/* ---- GROUP BY under a WHERE (not in the reference) ----
 * group_aggregate_where: SELECT key, count(*), sum(v), min(v), max(v) FROM t WHERE c0 IN [..)
 * AND c1 IN [..) ... GROUP BY key in one operator (mq_group_where_plan in
 * mq_device.h): what select_where -> fetch_column x 2 -> group_aggregate returns, without the
 * positions, the two fetched columns and the host round trip between them. `columns`, `lows`,
 * `highs` and `ncols` are select_where's, `keys` and `values` group_aggregate's: each a COLUMN
 * or an INT RESULT, all equally long; keys, values and any predicate column may be the same
 * object. Returns group_aggregate's five Results under the same ownership and shadow rules:
 * one tuple per distinct key that has a matching row, ascending: [0] keys (INT), [1] counts
 * (LONG), [2] sums (LONG), [3] minima (INT), [4] maxima (INT). No matching row gives five
 * empty Results and OK. No key bounds are passed, for group_aggregate's reason: the range of
 * the matching keys is found in one more pass over the predicates and the surviving key
 * lines, so a filter that narrows the keys to mq_group_dense_slots() values takes the dense
 * path. Measured on the device at 1e9 rows, the plan as called here (no
 * bounds) beats mq_where_positions -> mq_fetch x 2 -> mq_group_plan when half of the rows or
 * more match, ties at 10 % and loses below. Put the most selective predicate first. The operator runs on the calling device: a
 * column held as row shards drops them and is split again on next use. ERROR and NULL (a
 * "libmq:" line on stderr): no device, ncols outside 1..8, an argument of the wrong kind,
 * different lengths, 2^31 rows or more, a device failure. */
Result** group_aggregate_where(GeneralizedColumn** columns, int** lows, int** highs, int ncols,
                               GeneralizedColumn* keys, GeneralizedColumn* values, Status* ret_status);

/* ---- GROUP BY over several key columns (not in the reference) ----
 * group_aggregate_by: SELECT k0, .., count(*), sum(v), min(v), max(v) FROM t GROUP BY k0, ..
 * over nkeys = 1..MQ_GROUP_MAX_KEYS (4) key columns (mq_group_by_plan /
 * mq_group_by_write in mq_device.h). Each of keys[0..nkeys) and `values` is a COLUMN or an
 * INT RESULT, as group_aggregate takes them, all equally long; any of them may be the same
 * object. Returns a malloc'd array of nkeys + 4 Result* under group_aggregate's ownership
 * and shadow rules, one tuple per distinct (k0, .., k_{nkeys-1}), in ascending lexicographic
 * order with k0 the most significant: [0 .. nkeys) the key columns (INT), then counts (LONG),
 * sums (LONG), minima (INT) and maxima (INT). No rows give nkeys + 4 empty Results and OK.
 * No key bounds are passed, for group_aggregate's reason: every key column is read once more
 * for its range, and the product of the ranges picks the path (up to mq_group_dense_slots()
 * the one-pass table in LDS, up to 2^32 one packed column and the sort path). Runs on the
 * calling device; a column held as row shards drops them and is split again on next use.
 * ERROR and NULL (a "libmq:" line on stderr): group_aggregate's cases, nkeys outside 1..4, a
 * key space (the product of the columns' ranges) wider than 2^32. */
Result** group_aggregate_by(GeneralizedColumn** keys, int nkeys, GeneralizedColumn* values, Status* ret_status);

/* ---- GROUP BY over several key columns under a WHERE (not in the reference) ----
 * group_aggregate_by_where: SELECT k0, .., count(*), sum(v), min(v), max(v) FROM t WHERE c0 IN
 * [..) AND c1 IN [..) ... GROUP BY k0, .. in one operator (DESIGN.md §3.16;
 * mq_group_by_where_plan in mq_device.h): what select_where -> fetch_column x (nkeys + 1) ->
 * group_aggregate_by returns, without the positions, the fetched columns and the host round
 * trips between them. `columns`, `lows`, `highs` and `ncols` are group_aggregate_where's;
 * `keys`, `nkeys` and `values` are group_aggregate_by's, all as long as the predicate columns,
 * any of them the same object. Returns group_aggregate_by's nkeys + 4 Results under its
 * ownership and shadow rules: one tuple per distinct (k0, .., k_{nkeys-1}) that has a matching
 * row. No matching row gives nkeys + 4 empty Results and OK. No key bounds are passed, for
 * group_aggregate's reason: one more pass over the predicates and the surviving key lines
 * finds every key column's range over the matching rows, so a filter that narrows the tuples
 * to mq_group_dense_slots() takes the dense path. Measured on the device at 1e9 rows, the
 * plan as called here (no bounds) beats mq_where_positions -> mq_fetch x (nkeys + 1) ->
 * mq_group_by_plan when the leading predicate passes half of the rows or more (0.59-0.86 of its
 * time) and loses below (1.2-2.6). Put the most selective predicate first. Runs on the calling device; a column held as row shards drops them and is split again
 * on next use. ERROR and NULL (a "libmq:" line on stderr): group_aggregate_where's and
 * group_aggregate_by's cases. */
Result** group_aggregate_by_where(GeneralizedColumn** columns, int** lows, int** highs, int ncols,
                                  GeneralizedColumn** keys, int nkeys, GeneralizedColumn* values,
                                  Status* ret_status);

/* ---- GROUP BY an attribute of a joined dimension (not in the reference) ----
 * group_aggregate_join: SELECT d.attr, count(*), sum(f.v), min(f.v), max(f.v) FROM f JOIN d ON
 * f.fkey = d.key WHERE f.c0 IN [..) AND ... GROUP BY d.attr in one operator (DESIGN.md §3.18;
 * mq_keymap_build and mq_group_join_plan in mq_device.h): what hash_join -> fetch_column x 2 ->
 * group_aggregate returns behind a select_where, without the pair list, the gathered columns
 * and the host round trips between them. `columns`, `lows`, `highs` and `ncols` are
 * select_where_in's: ncols is 0..8, and with ncols == 0 the first three may be NULL. `fkeys`
 * (the fact table's foreign key) and `values` are a COLUMN or an INT RESULT as long as the
 * columns; `dim_keys` and `dim_attrs` are a COLUMN or an INT RESULT, equally long (below 2^31),
 * and dim_keys holds every key once (a primary key). A fact row whose key has no partner is
 * dropped (an inner join); an empty dimension gives five empty Results and OK. Returns
 * group_aggregate's five Results under its ownership and shadow rules, one tuple per attribute
 * with a joined row, ascending: [0] attributes (INT), [1] counts (LONG), [2] sums (LONG),
 * [3] minima (INT), [4] maxima (INT). The key map (bitmap, rank directory and attributes over
 * the span of dim_keys, up to 1.5 GiB + 4 bytes a key) is built per call and freed before
 * returning. No attribute bounds are passed and none are searched for: the map knows its
 * attributes' range. Runs on the calling device; a column held as row shards drops them and is
 * split again on next use. ERROR and NULL (a "libmq:" line on stderr): no device, ncols outside
 * 0..8, an argument of the wrong kind, different lengths, 2^31 rows or more, a key that occurs
 * twice in dim_keys, a device failure. Not measured on a device yet. */
Result** group_aggregate_join(GeneralizedColumn** columns, int** lows, int** highs, int ncols /* 0..8 */,
                              GeneralizedColumn* fkeys, GeneralizedColumn* dim_keys,
                              GeneralizedColumn* dim_attrs, GeneralizedColumn* values, Status* ret_status);

/* ---- GROUP BY over several joined dimensions (not in the reference) ----
 * group_aggregate_star: SELECT d1.a, d2.b, f.k, count(*), sum(f.v), min(f.v), max(f.v) FROM f
 * JOIN d1 ON f.k1 = d1.key JOIN d2 ON f.k2 = d2.key [JOIN d3 ... only as a filter] WHERE f.c0 IN
 * [..) AND ... GROUP BY d1.a, d2.b, f.k in one operator (mq_group_star_plan in
 * mq_device.h). `columns`, `lows`, `highs` and `ncols` are group_aggregate_join's. `fkeys`,
 * `dim_keys` and `dim_attrs` each hold `nterms` (1..4) entries; term t is fkeys[t], a fact
 * column, and
 *   dim_keys[t] == NULL (dim_attrs[t] must be NULL too): fkeys[t] itself is a group key;
 *   dim_keys[t] and dim_attrs[t]: a dimension, joined on fkeys[t] = dim_keys[t], whose attribute
 *       is a group key (a key map built per call; dim_keys[t] holds every key once);
 *   dim_keys[t] alone: a dimension joined only as a filter (a key set built per call): the row
 *       is kept when fkeys[t] is among dim_keys[t]; no group key.
 * The terms must give nkeys = 1..4 group keys, in the order of the terms, the first most
 * significant. Every fkeys entry and `values` are a COLUMN or an INT RESULT as long as the
 * columns; dim_keys[t] and dim_attrs[t] are a COLUMN or an INT RESULT, equally long (below 2^31).
 * A fact row whose key has no partner in some dimension is dropped (inner joins); an empty
 * dimension gives empty Results and OK. Returns group_aggregate_by's nkeys + 4 Results under its
 * ownership and shadow rules (with nkeys == 1 group_aggregate's five): the key columns (INT) in
 * the order of the terms, then counts (LONG), sums (LONG), minima (INT), maxima (INT), one tuple
 * per distinct key tuple with a joined row, ascending lexicographically. The ranges run first,
 * then the terms in the order given: put the most selective first. Every map and set is freed
 * before returning, on every path. No key bounds are passed: a dimension's attribute range is
 * known from its map, and a plain group key costs one more read of its whole column. Runs on
 * the calling device; a column held as row shards drops them and is split again on next use.
 * ERROR and NULL (a "libmq:" line on stderr): no device, ncols outside 0..8, nterms outside
 * 1..4, no or more than four group keys, dim_attrs without dim_keys, an argument of the wrong
 * kind, different lengths, 2^31 rows or more, a key that occurs twice in a mapped dim_keys[t], a
 * key space wider than 2^32, a device failure. Not measured on a device yet. */
Result** group_aggregate_star(GeneralizedColumn** columns, int** lows, int** highs, int ncols /* 0..8 */,
                              GeneralizedColumn** fkeys, GeneralizedColumn** dim_keys,
                              GeneralizedColumn** dim_attrs, int nterms /* 1..4 */,
                              GeneralizedColumn* values, Status* ret_status);

/* ---- Several expression aggregates over a star query's groups (not in the reference) ----
 * group_aggregate_measures: group_aggregate_star with nmeas (1..4) measures in place of `values`
 * (mq_group_measures_plan in mq_device.h). Measure m is meas_a[m] (ops[m] ==
 * MQ_MEAS_COL, and meas_b[m] must be NULL, as may meas_b itself when no measure is binary) or
 * meas_a[m] + / - / * meas_b[m] (MQ_MEAS_ADD / MQ_MEAS_SUB / MQ_MEAS_MUL), computed exactly in 64
 * bits per row. Every operand is a COLUMN or an INT RESULT as long as the columns; operands may
 * repeat and may be term or predicate columns. The other arguments and the ownership, shadow and
 * error rules are group_aggregate_star's. Returns nkeys + 1 + 3 * nmeas Results: the key columns
 * (INT), the counts (LONG), then per measure its sums (modulo 2^64), minima and maxima (LONG
 * each), one tuple per distinct key tuple with a joined row, ascending lexicographically. ERROR
 * and NULL also for nmeas outside 1..4, an op outside the four, a missing or a superfluous
 * meas_b[m]. Not measured on a device yet. */
Result** group_aggregate_measures(GeneralizedColumn** columns, int** lows, int** highs, int ncols /* 0..8 */,
                                  GeneralizedColumn** fkeys, GeneralizedColumn** dim_keys,
                                  GeneralizedColumn** dim_attrs, int nterms /* 1..4 */,
                                  GeneralizedColumn** meas_a, GeneralizedColumn** meas_b /* entries NULL for COL */,
                                  const int* ops, int nmeas /* 1..4 */, Status* ret_status);

/* ---- COUNT(DISTINCT v) per group under a WHERE (not in the reference) ----
 * group_count_distinct: SELECT k0, .., count(DISTINCT v) FROM t WHERE c0 IN [..) AND .. GROUP BY
 * k0, .. in one operator (mq_group_distinct_plan in mq_device.h). The arguments
 * are group_aggregate_by_where's (Columns or INT Results, all equally long, any of them the same
 * object); with ncols == 0 every row matches and `columns`, `lows` and `highs` may be NULL.
 * Returns a malloc'd array of nkeys + 1 Results under group_aggregate's ownership and shadow
 * rules: the key columns (INT, with HBM shadows), then the distinct counts (LONG), one tuple per
 * distinct (k0, .., k_{nkeys-1}) that has a matching row, in ascending lexicographic order. No
 * matching row gives nkeys + 1 empty Results and OK. No bounds are passed, for group_aggregate's
 * reason: the plan finds the keys' and the values' ranges over the matching rows itself. Runs on
 * the calling device; a column held as row shards drops them and is split again on next use.
 * ERROR and NULL (a "libmq:" line on stderr): group_aggregate_by_where's cases, with ncols 0
 * allowed. Not measured on a device yet. */
Result** group_count_distinct(GeneralizedColumn** columns, int** lows, int** highs, int ncols /* 0..8 */,
                              GeneralizedColumn** keys, int nkeys, GeneralizedColumn* values, Status* ret_status);

/* ---- HAVING, ORDER BY an aggregate and LIMIT over group results (not in the reference) ----
 * group_top_k: the tail of a GROUP BY query (mq_topk64 in mq_device.h). `groups`
 * is the array any group_aggregate* returned: nresults equally long Results, each INT or LONG
 * (nkeys + 4 of them, or nkeys + 1 + 3 * nmeas from group_aggregate_measures). Tuple i passes
 * when having_by is -1 or *low <= groups[having_by][i] < *high holds (either bound NULL:
 * unbounded). The m = min(k, passing) first passing tuples of a stable sort by
 * groups[order_by], ascending or descending, equal values in input (key) order both ways, are
 * returned; order_by == -1 keeps the input order (HAVING and LIMIT alone; `descending` is
 * ignored). Returns a new malloc'd array of nresults Result* with malloc'd payloads the caller
 * frees, each of m tuples and of its input's data type; INT payloads keep an HBM shadow as
 * every INT Result does. INT inputs are read through their shadow where they have one, LONG
 * payloads are uploaded (they are small); ordering and gathers run on the device. The inputs
 * are not consumed and not changed. k == 0 or no groups give empty Results and OK. ERROR and
 * NULL (a "libmq:" line on stderr): no device, nresults < 1, an index out of range, a Result
 * that is neither INT nor LONG, unequal lengths, 2^31 tuples or more, a device failure. */
Result** group_top_k(Result** groups, int nresults, int order_by /* index into groups, or -1: keep key order */,
                     bool descending, size_t k, int having_by /* index, or -1 */,
                     const long* low, const long* high /* NULL: unbounded; low <= v < high */,
                     Status* ret_status);

/* ---- libmq residency control (not in the reference) ----
 * A device copy of host memory (a Column's rows, a Result payload, an index's
 * arrays) is reused by later operators only while a write guard proves the host
 * memory unchanged: the whole pages inside it are read-only, the
 * first write into them faults once and marks the copy stale. Guarded are the
 * reference's column files (any writable file-backed mapping, e.g. start_data's
 * MAP_SHARED column files, or a memfd) and the payloads libmq allocates when glibc
 * serves them with mmap. Any other memory is uploaded again by each operator that
 * reads it. MQ_GUARD=0 turns the guards off (every copy single-use). */
/* Use an existing device copy of column->data (row_count int32 rows in HBM); the
 * caller keeps ownership of d_data and must keep it alive while attached (attached
 * copies are trusted: not guarded). */
int mq_column_attach(Column* column, const int32_t* d_data);
/* Upload column->data now (otherwise done lazily on first use). */
int mq_column_upload(Column* column);
/* Forget the device copy (call after insert_row / reorder / remap of the column). */
void mq_column_invalidate(Column* column);
/* Device pointer of a libmq-produced Result's shadow copy, or NULL. */
const void* mq_result_device_ptr(const Result* result);
/* Row shards: columns of at least min_rows rows are split into `shards`
 * contiguous row ranges, range g resident on device devices[g % ndev] (ndev = 0: the
 * primary device + g, modulo the device count) and served by a host thread and stream
 * of its own; select_column, fetch_column, sum/avg/min/max and shared_select then run
 * on every shard and concatenate / fold in shard order. Replaces the MQ_SHARDS /
 * MQ_DEVICES / MQ_SHARD_MIN_ROWS environment (read at first use); drops every sharded
 * copy first. shards <= 0 returns to the environment's layout. Several shards may
 * share one device (a rehearsal of the split on a one-GPU machine). */
int mq_shard_config(int shards, const int* devices, int ndev, uint64_t min_rows);
/* The current layout: returns the shard count G, devices[g] (up to max) its devices. */
int mq_shard_devices(int* devices, int max);
/* hash_join (query.c:652-696) key-partitioned over the G shards (DESIGN.md
 * §6; hash_join / nested_loop_join take it for probe sides of at least min_rows rows).
 * Shard g holds build rows (d_c1[g], d_p1[g], n1[g]) and probe rows (d_c2[g], d_p2[g],
 * n2[g]) on its device, the ranges of each side in row order (any split). On return
 * shard g's device holds d_out1[g] / d_out2[g]: the h_m[g] pairs of probe rows of range
 * g, in the reference's order; their concatenation over g is hash_join's output. The
 * outputs are pool memory (mq_pool_free). Starts the shard workers if needed.
 * Stream contract: the inputs may still be being written by work the caller queued on
 * ANY stream of the shard devices, the null stream included: mq_shard_join first waits
 * for every shard device to go idle (mq_device_sync on each worker), because its
 * workers run on non-blocking streams of their own that would not wait for that work.
 * On return every output is complete (each worker has synchronised its stream). Work
 * the caller queues concurrently from other threads while the call runs is not
 * ordered against it. */
int mq_shard_join(const int32_t* const* d_c1, const int32_t* const* d_p1, const uint64_t* n1,
                  const int32_t* const* d_c2, const int32_t* const* d_p2, const uint64_t* n2,
                  int32_t** d_out1, int32_t** d_out2, uint64_t* h_m);
/* Host wall ms of the last partitioned join's phases: partition, exchange + local join,
 * return exchange + place, total. */
void mq_shard_join_times(double* ms);
/* Test hook (no reference counterpart): every device allocation of the next
 * mq_shard_join calls' phase `phase` fails with MQ_ENOMEM (1 partition, 2 exchange + local
 * join, 3 return + place, 4 the one-shard join; 0 turns it off). The error paths drain
 * every worker's stream before buffers go back to the pool. */
void mq_shard_join_inject_failure(int phase);
/* Drop every cached device copy. */
void mq_release_all(void);
/* Residency counters since load (tests and the bench read them). */
typedef struct mq_residency {
    uint64_t column_uploads, column_bytes;  /* H2D uploads of column rows */
    uint64_t result_uploads, result_bytes;  /* H2D uploads of Result payloads */
    uint64_t guards_armed, guard_clean, guard_stale, guards_live;
    uint64_t remap_probe;                   /* 1: a remapped range is told apart (MADV_POPULATE_WRITE) */
    uint64_t columns_resident, shadows_resident, shadow_bytes;
    /* row shards (MQ_SHARDS): shard count, sharded columns and result shadows held,
     * sharded operator calls served, sharded column uploads */
    uint64_t shards, shard_columns, shard_shadows, shard_ops, shard_uploads;
} mq_residency;
void mq_residency_stats(mq_residency* out);
/* Seconds spent in host<->device copies by the query API since the last reset. */
double mq_transfer_seconds(int reset);

#ifdef __cplusplus
}
#endif
#endif
