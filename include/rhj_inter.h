/*
 * rhj_inter.h — device-resident intermediate results: the "next" rows of SURVEY.md §8(f).
 *
 * The reference keeps a query's intermediate result (`inter_res`: per active relation one
 * array of row ids, structs.h:97-111) on the host and rebuilds it after every operator with
 * gathers (inter_res.c, the helper half of filter.c): 71 % of the `small` workload's run
 * time.  Around the hot path that means H2D of both join inputs and D2H of every match
 * list per join.  This header is the reference's own inter_res.h / filter.h:15 interface —
 * same names, same signatures, same struct layouts — implemented so that the row-id tables,
 * the materialised join inputs and the result lists never leave the GPU:
 *
 *   inter_data.table[rel]   device pointer (u64[num_tuples]) or NULL       structs.h:97-101
 *   relation.tuples         device pointer, for relations from GetRelation structs.h:25-29
 *   result.buff             device pointer, ONE node holding all elements  structs.h:37-43
 *
 * The structs themselves, `num_tuples`, `current_load`, `next` and the NULL-ness of
 * `table[rel]` stay host-readable, which is all the reference's query.c looks at
 * (query.c:334-465).  A maintainer switches the engine to this mode by NOT compiling
 * inter_res.c and filter.c (and, for device-side loading and statistics, relation_map.c)
 * and linking librhj.so instead; with the
 * reference's own inter_res.c in the link these definitions are simply never called and
 * RadixHashJoin()/Filter() keep their host-memory behaviour.  RadixHashJoin(), Filter(),
 * FreeRelation(), FreeResult() and GetResultNum() recognise device-resident arguments by
 * identity (objects created here are registered), not by a global switch.
 *
 * Semantics follow inter_res.c line by line (cited per function), with two documented
 * departures where the reference's code is broken: SelfJoin uses the
 * mapped relation's tuple count and pushes the inter_res position (inter_res.c:252,259 use
 * the wrong index); InsertSingleRowIdsToInterResult appends a node to the LAST node instead
 * of dereferencing the NULL it just walked to (filter.c:83-88).
 */
#ifndef RHJ_INTER_H
#define RHJ_INTER_H

#include "rhj.h"

#ifdef __cplusplus
extern "C" {
#endif

/* structs.h:178-203: what CalculateQueryResults / PrintNullResults read of a query */
typedef struct rhj_query_string_array {
    char **data;
    int    num_of_elements;
} rhj_query_string_array;

typedef struct rhj_batch_listnode {
    int                         num_of_relations;
    int                        *relations;
    void                       *predicate_list;      /* predicates_listnode*, not used here */
    rhj_query_string_array     *views;
    struct rhj_batch_listnode  *next;
} rhj_batch_listnode;

/* inter_res.h:5-17 */
int  InitInterData(rhj_inter_data **head, int num_of_relations, int num_tuples);     /* inter_res.c:10-15  */
void FreeInterData(rhj_inter_data *head, int num_of_relations);                      /* inter_res.c:17-24  */
int  InitInterResults(rhj_inter_res **head, int num_of_relations);                   /* inter_res.c:26-32  */
void PrintInterResults(rhj_inter_res *head);                                         /* inter_res.c:154-173 */
void FreeInterResults(rhj_inter_res *var);                                           /* inter_res.c:175-180 */

/* inter_res.h:26: rebuild the node after a join; res pairs index the node's rows on the
 * side that was already active (inter_res.c:34-152) */
int  InsertJoinToInterResults(rhj_inter_res *head, int ex_rel_num, int new_rel_num, rhj_result *res);

/* inter_res.h:33,41: materialise {value = col[table[rel][i]] or col[i], row_id = i}
 * (inter_res.c:182-231) */
rhj_relation *GetRelation(int given_rel, int column, rhj_inter_res *inter, rhj_relation_map *map, int *query_relations);
rhj_relation *ScanInterResults(int given_rel, int column, rhj_inter_res *inter, rhj_relation_map *map, int *query_relations);

/* inter_res.h:44 (inter_res.c:234-263, intended semantics, see above) */
rhj_result *SelfJoin(int given_rel, int column1, int column2, rhj_inter_res **inter, rhj_relation_map *map,
                     int *query_relations);

/* inter_res.h:48,51 (inter_res.c:265-318) */
void MergeInterNodes(rhj_inter_res **inter);
void Merge(rhj_inter_res **head, rhj_inter_res **node, int rel_num);

/* inter_res.h:55,58: wrap-around u64 sums of the views, printed as the reference prints them
 * (inter_res.c:320-350) */
void CalculateQueryResults(rhj_inter_res *inter, rhj_relation_map *map, rhj_batch_listnode *query);
void PrintNullResults(rhj_batch_listnode *query);

/* inter_res.h:61,64,68 (inter_res.c:352-428) */
int  AreActiveInInter(rhj_inter_res *inter, int rel1, int rel2);
int  JoinInterNode(rhj_inter_res **inter, rhj_relation_map *rel_map, int relation1, int column1, int relation2,
                   int column2, int *relations);
void CartesianInterResults(rhj_inter_res **inter);

/* filter.h:15 (filter.c:11-89) */
int  InsertSingleRowIdsToInterResult(rhj_inter_res **head, int relation_num, rhj_result *res);

/* relation_map.h:10-16: map the relation files (header u64 tuples, u64 columns,
 * then column-major u64 data, relation_map.c:39-50), copy every column to the device once — the
 * copies Filter()/GetRelation()/CalculateQueryResults() use — and compute the optimiser's column
 * statistics there: l = min, u = max, f = tuples, d = distinct values counted with the reference's
 * flag array including its cap (range above 50 000 000 folds modulo 5 000 000, relation_map.c:66-84). */
typedef struct rhj_relation_listnode {       /* structs.h:86-91 */
    char                         *filename;
    int                           fd;
    struct rhj_relation_listnode *next;
} rhj_relation_listnode;
int  InitRelationMap(rhj_relation_listnode *head, rhj_relation_map *rel_map);   /* relation_map.c:13-88  */
void FreeRelationMap(rhj_relation_map *rel_map, int map_size);                   /* relation_map.c:90-98  */
void PrintRelationMap(rhj_relation_map *rel_map, int map_size);                  /* relation_map.c:100-115 */

/* ---- device entry points behind them (tests and bench call these directly) ---------- */

/* dst[t][i] = src[t][idx[i * idx_stride]] for t < ntab (idx_stride 2 walks one side of a pair
 * list); src[t] == NULL writes the index itself.  All pointers are device pointers. */
int rhj_gather_tables_device(uint64_t *const *dst, const uint64_t *const *src, int ntab, const uint64_t *idx,
                             int idx_stride, uint64_t n);
/* tuples[i] = {col[sel ? sel[i] : i], i} */
int rhj_build_relation_device(const uint64_t *d_col, const uint64_t *d_sel, uint64_t n, rhj_tuple *d_tuples);
/* wrap-around sum of col[sel[i]] (sel may be NULL) */
int rhj_sum_gather_device(const uint64_t *d_col, const uint64_t *d_sel, uint64_t n, uint64_t *sum);
/* up to 8 such sums in one launch (CalculateQueryResults: all views of a query) */
int rhj_sum_views_device(int views, const uint64_t *const *d_cols, const uint64_t *const *d_sels, const uint64_t *ns, uint64_t *sums);
/* ascending i with colA[selA ? selA[i] : i] == colB[selB ? selB[i] : i] */
int rhj_filter_eq2_device(const uint64_t *d_colA, const uint64_t *d_selA, const uint64_t *d_colB, const uint64_t *d_selB,
                          uint64_t n, uint64_t *d_out, uint64_t *hits);
/* min, max and the reference's distinct-value estimate of a device column (n >= 1).  A range u - l + 1 below
 * 50 000 000 counts one flag per value; 50 000 000 or more folds (u - l) modulo 5 000 000.  The full range
 * (l = 0, u = 2^64 - 1), whose u - l + 1 wraps to 0, is folded the same way; the reference's code is undefined
 * there (it indexes a calloc of 0 entries, relation_map.c:64-74). */
int rhj_column_stats_device(const uint64_t *d_col, uint64_t n, uint64_t *l, uint64_t *u, double *d);

/* Many row-id rebuilds and view sums in one call: what consumes a pair list (the two gathers of InsertJoinToInterResults, the
 * sums of CalculateQueryResults) for a whole batch of queries, one kernel launch and one stream synchronisation per chunk of
 * up to 4096 items and 2^24 tiles of 2048 rows, in call order.  One item applies one index list to up to
 * RHJ_APPLY_MAX_TERMS terms.  For row i < n and term t:
 *     p = d_idx ? d_idx[i * idx_stride + side_t] : i
 *     q = d_src_t ? d_src_t[p] : p
 *     if d_dst_t:  d_dst_t[i] = q
 *     if d_col_t:  sum_t += d_col_t[q]          (u64, wrap-around)
 * so an item is the rebuild through one or both sides of a pair list (idx_stride 2, side 0 / 1, d_src the old vector or NULL
 * for the fresh relation), the rebuild through a filter's hit list (idx_stride 1), the plain view sum (d_idx NULL, d_src the
 * row-id vector) or the view sum through the last join's pairs with no table written (d_dst NULL).
 *
 * d_dst[0..n) of every writing term holds the gathered ids and nothing at or beyond d_dst[n] is written; every sum is exact
 * modulo 2^64.  Inputs may be shared between items and between terms; outputs must not overlap each other or any input of the
 * call.  Every pointer needs 8-byte alignment and no more (pairs + 1 with stride 2 is a legal d_idx).  The caller guarantees
 * that every p indexes its d_src and every q its d_col.  An item with n == 0 has rc 0, sums 0 and path 0 and launches nothing;
 * a batch of 0 items returns 0 without touching a device.
 *
 * The whole batch is validated before anything is launched: idx_stride outside {1, 2}, nterms outside
 * 1..RHJ_APPLY_MAX_TERMS, a side outside 0..idx_stride - 1, side != 0 with d_idx == NULL, a term with neither d_dst nor d_col,
 * or n above 2^35 give that item rc -3; then nothing runs and the call returns -3.  Otherwise 0, or a negative value on a HIP
 * error.  rhj_last_stats() afterwards: n_r the rows summed over the items, units the items launched, ms_total the whole call
 * (timing level >= 1), reserved 8. */
#define RHJ_APPLY_MAX_TERMS 8
typedef struct rhj_apply_term {
    const uint64_t *d_src;   /* NULL: q = p */
    uint64_t       *d_dst;   /* NULL: nothing written for this term */
    const uint64_t *d_col;   /* NULL: no sum */
    uint64_t        sum;     /* out; 0 without d_col */
    int             side;    /* word of an index row, 0 .. idx_stride - 1 */
} rhj_apply_term;
typedef struct rhj_apply_desc {
    const uint64_t *d_idx;   /* NULL: p = i */
    uint64_t        n;
    int             idx_stride;          /* 1 or 2 */
    int             nterms;              /* 1 .. RHJ_APPLY_MAX_TERMS */
    rhj_apply_term  terms[RHJ_APPLY_MAX_TERMS];
    int             rc;      /* out */
    int             path;    /* out: 8 (0 for an item that launched nothing) */
} rhj_apply_desc;
int rhj_apply_batch_device(rhj_apply_desc *items, uint64_t n);

/* Many two-column equalities in one call (csrc/rhj_eq2_batch.hip.h): what SelfJoin and the same-node branch of JoinInterNode
 * (inter_res.c:234-263, :363-389) need for a whole batch of queries.  d_out[0..hits) gets the ascending i in [0, n) with
 * colA[selA ? selA[i] : i] == colB[selB ? selB[i] : i]; nothing at or beyond d_out[hits] is written; hits is exact, also with
 * d_out == NULL (count only).  A one-item batch returns bit for bit what rhj_filter_eq2_device returns.  Inputs may be shared
 * between items and between the two sides of one item (the same vector on both sides is the SelfJoin form); outputs must not
 * overlap; every pointer needs only 8-byte alignment (a side takes the 16-byte loads only when the vector it scans - its sel,
 * or its column without one - starts on a 16-byte boundary).  The items rhj_filter_batch_takes(n) names (1..4 194 304 rows) run
 * together in two launches (masks, index lists) and one stream synchronisation per chunk of at most 4096 items and 1 GiB of
 * masks, in call order, whatever their number (path 9); a larger item is run alone inside the same call by the single call's
 * kernels (path 0).  n == 0: rc 0, hits 0, path 0, nothing launched; a batch of 0 items returns 0 without touching a device.
 * The whole batch is validated before anything is launched: a NULL column with n > 0 gives that item rc -3, nothing runs and
 * the call returns -3.  Otherwise 0, <0 on a HIP error.  rhj_last_stats() afterwards: n_r the rows and matches the hits summed
 * over the items, units the items that went through the batched launches, ms_total the whole call (timing level >= 1),
 * reserved 9. */
typedef struct rhj_eq2_desc {
    const uint64_t *d_colA, *d_selA;   /* sel NULL: the column's rows 0..n) */
    const uint64_t *d_colB, *d_selB;
    uint64_t        n;
    uint64_t       *d_out;             /* capacity n; NULL: count only */
    uint64_t        hits;              /* out */
    int             rc;                /* out */
    int             path;              /* out: 9 the batched launches, 0 run alone or nothing launched */
} rhj_eq2_desc;
int rhj_filter_eq2_batch_device(rhj_eq2_desc *items, uint64_t n);

/* A batch of queries run level by level through the four batches above: one rhj_filter_batch_device call, then per join level
 * at most one rhj_filter_eq2_batch_device call, at most two rhj_join_cols_batch_device calls and one rhj_apply_batch_device
 * call, with no single call in between.  The relations are device-resident column stores; nothing but the descriptors and the
 * answers crosses the bus.
 *
 * Per query (the reference's executor, query.c:334-465, without its optimiser): the filters restrict their bindings; the join
 * predicates are applied left to right, in the order given; the views are summed over the final rows modulo 2^64.  A predicate
 * whose two bindings already sit in one intermediate node, or are the same binding, is a two-column equality over that node's
 * rows (SelfJoin / JoinInterNode's same-node branch); every other predicate is a join of the two nodes on the two columns read
 * through the bindings' row-id vectors, after which the two nodes are one.  rows is the number of rows of the final result;
 * rows == 0 is the case the reference prints NULL for every view in (sums are 0 then).  Sums do not depend on the order of the
 * rows, so the answers are the same at every radix width and order mode.
 *
 * All filters of one binding are ONE conjunctive rhj_filter_desc (at most RHJ_FILTER_MAX_TERMS of them); a query without a
 * join predicate sums its views through its one binding's vector in the first apply call.  A query whose intermediate result
 * becomes empty is finished there and adds no further item.  Joins get room for max(nR, nS) pairs; those that need more run
 * once more, in one second call per level, with room for their counts.
 *
 * The whole batch is validated before a device is touched: nrels outside 1..RHJ_QUERY_MAX_RELS, nviews outside
 * 1..RHJ_QUERY_MAX_VIEWS, a negative count, a binding, relation or column index out of range, a used column that is NULL in a
 * relation with rows, an operator outside '<', '>', '=', more than RHJ_FILTER_MAX_TERMS filters on one binding, or bindings
 * that are not all in one node after the last predicate (a cross product, CartesianInterResults: taken only with
 * rhj_set_query_products on, below, and then as the product of its components' answers, never materialised) give that
 * query rc -3; then nothing runs, no sums or rows are written and the call returns -3.  n == 0 returns 0.  Otherwise 0, or a
 * negative value on a HIP error.  The call holds the library lock throughout and keeps its intermediate vectors in workspace
 * buffers that grow and stay (rhj_release() frees them).  rhj_last_stats() afterwards: n_r the queries, matches the final rows
 * summed over them, ms_total the whole call (timing level >= 1), reserved 10. */
typedef struct rhj_device_relation {          /* a device-resident column store */
    uint64_t num_tuples, num_columns;
    const uint64_t *const *d_columns;         /* host array of num_columns device pointers */
} rhj_device_relation;
typedef struct rhj_query_filter { int rel, col; char op; uint64_t value; } rhj_query_filter;  /* rel = binding; value already converted, as rhj_filter_device */
typedef struct rhj_query_join   { int relA, colA, relB, colB; } rhj_query_join;               /* rel = binding */
typedef struct rhj_query_view   { int rel, col; } rhj_query_view;                             /* rel = binding */
#define RHJ_QUERY_MAX_RELS  8
#define RHJ_QUERY_MAX_VIEWS 8
typedef struct rhj_query_desc {
    int nrels;    const int *rels;                   /* binding -> index into the relation array; a relation may be bound twice */
    int nfilters; const rhj_query_filter *filters;
    int njoins;   const rhj_query_join *joins;       /* executed left to right, in this order: the caller's optimiser chose it */
    int nviews;   const rhj_query_view *views;
    uint64_t sums[RHJ_QUERY_MAX_VIEWS];              /* out: wrap-around u64 sums */
    uint64_t rows;                                   /* out: rows of the final result; 0: the reference prints NULL for every view */
    int rc;                                          /* out */
} rhj_query_desc;
int rhj_query_batch_device(const rhj_device_relation *rels, int nrel, rhj_query_desc *queries, uint64_t n);
/* The validation of one query, a pure function that needs no device: njoins, or -3.  kinds, when given, receives per step
 * 0 for a join and 1 for a two-column equality (njoins entries; what was written before a -3 is not meaningful).  rels may
 * be NULL: then relation and column indices are only checked against nrel and for sign. */
int rhj_query_levels(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, int *kinds);
/* What the last rhj_query_batch_device call of this process issued: the join levels (the largest njoins) and the calls of
 * each inner batch (join_calls the first calls of the levels, join_reruns the second ones). */
typedef struct rhj_query_batch_info { uint32_t levels, filter_calls, eq2_calls, join_calls, join_reruns, apply_calls; } rhj_query_batch_info;
const rhj_query_batch_info *rhj_query_batch_last_info(void);

/* The statistics of many columns in one call (csrc/rhj_stats_batch.hip.h): what InitRelationMap needs for every column of every
 * relation, and what a caller of rhj_query_batch_device needs for its own optimiser.  Every column gets, bit for bit, what
 * rhj_column_stats_device returns (relation_map.c:53-84): l the minimum and u the maximum, compared unsigned; d the number of
 * distinct v - l when u - l + 1 < 50 000 000, else the number of distinct (v - l) % 5 000 000 (the wrapped full range too).
 * Every column of at least one row goes through the batched launches (path 11), three launches and two stream
 * synchronisations per chunk of at most 4096 columns, 2^24 tiles of 2048 rows and 256 MiB of flag bitmaps (one bit a flag;
 * the widest column needs 6.25 MB), in call order; columns whose bitmaps did not fit their chunk's arena keep their extremes
 * and are marked and counted in a following chunk of two launches and one synchronisation.  Columns may be shared between
 * items and the same column may appear twice; a column needs 8-byte alignment and no more.  n == 0: l = u = 0, d = 0, rc 0,
 * path 0, nothing launched; a batch of 0 columns returns 0 without touching a device.
 *
 * The whole batch is validated before anything is launched: a NULL column with n > 0, or n above 2^35, gives that item rc -3;
 * then nothing runs, no l, u or d is written and the call returns -3.  Otherwise 0, or a negative value on a HIP error.
 * rhj_last_stats() afterwards: n_r the rows summed over the columns, units the columns launched, ms_total the whole call
 * (timing level >= 1), reserved 11. */
typedef struct rhj_colstats_desc {
    const uint64_t *d_col; uint64_t n;   /* a device column, 8-byte aligned and no more (col + 1 is legal) */
    uint64_t l, u;                       /* out: min, max */
    double   d;                          /* out: the reference's distinct-value estimate */
    int      rc;                         /* out */
    int      path;                       /* out: 11 the batched launches, 0 nothing launched */
} rhj_colstats_desc;
int rhj_column_stats_batch_device(rhj_colstats_desc *cols, uint64_t n);
/* flags the estimate of a column with these extremes counts over: u - l + 1 when that is below 50 000 000, else 5 000 000
 * (also for l = 0, u = 2^64 - 1, whose u - l + 1 wraps to 0); 0 for l > u.  Pure function, needs no device. */
uint64_t rhj_column_stats_flags(uint64_t l, uint64_t u);
typedef struct rhj_colstats_batch_info { uint32_t chunks, columns; } rhj_colstats_batch_info;   /* of the last call: chunks run, columns that went through them */
const rhj_colstats_batch_info *rhj_column_stats_batch_last_info(void);

/* The row count and the view sums of many final joins in one call, without their pairs (csrc/rhj_join_sum_batch.hip.h): what a
 * query's last join and the sums behind it need.  Per item, matches and every sum are, as integers, what
 * rhj_join_cols_batch_device on the same four pointers with enough room, followed by rhj_apply_batch_device over its pairs
 * (idx_stride 2, the same side, d_src and d_col, d_dst NULL) give: for a join on keyR(i) == keyS(j),
 *     matches                = sum over keys k of cntR(k) * cntS(k)
 *     sum of a term, side 0  = sum over i of cntS(keyR(i)) * d_col[d_src ? d_src[i] : i]
 *     sum of a term, side 1  = sum over j of cntR(keyS(j)) * d_col[d_src ? d_src[j] : j]
 * which is linear in nR + nS and needs no pair buffer, no capacity and no second call.  Sums are exact modulo 2^64; matches is
 * exact (below 2^64: a side has fewer than 2^32 rows).  Neither depends on the radix width or the order mode.
 *
 * Every item with two non-empty sides runs in the launches of its chunk (path 12): three launches (insert the smaller side's
 * keys into the item's hash table - R on a tie -, count the other side's, sum) and one stream synchronisation per chunk of at
 * most 4096 items, 2^24 tiles of 2048 rows and 1 GiB of tables (16 bytes a slot, the smallest power of two of slots that is at
 * least twice the smaller side's rows), in call order; a chunk takes its first item whatever that needs.  Inputs may be shared
 * between items, between sides and between terms; every pointer needs 8-byte alignment and no more; the caller guarantees that
 * every index indexes its array.  An item with an empty side has rc 0, matches 0, sums 0 and path 0 and launches nothing; a
 * batch of 0 items returns 0 without touching a device.
 *
 * The whole batch is validated before anything is launched: a NULL key column with a non-zero size, nterms outside
 * 0..RHJ_JOIN_SUM_MAX_TERMS, a side outside 0..1, a term with a NULL d_col, or a side of 2^32 rows or more give that item
 * rc -3; then nothing runs, no matches or sum is written and the call returns -3.  Otherwise 0, or a negative value on a HIP
 * error.  rhj_last_stats() afterwards: n_r and n_s the rows summed over the items, matches the pairs summed modulo 2^64, units
 * the items launched, ms_total the whole call (timing level >= 1), reserved 12. */
#define RHJ_JOIN_SUM_MAX_TERMS 8
typedef struct rhj_join_sum_term {
    const uint64_t *d_src;   /* NULL: q = p */
    const uint64_t *d_col;   /* never NULL */
    uint64_t        sum;     /* out */
    int             side;    /* 0: p = i (R's position), 1: p = j (S's position) */
} rhj_join_sum_term;
typedef struct rhj_join_sum_desc {
    const uint64_t *d_colR, *d_selR; uint64_t nR;     /* tuple i of R = { d_colR[d_selR ? d_selR[i] : i], i } */
    const uint64_t *d_colS, *d_selS; uint64_t nS;
    int               nterms;                          /* 0 .. RHJ_JOIN_SUM_MAX_TERMS; 0: count only */
    rhj_join_sum_term terms[RHJ_JOIN_SUM_MAX_TERMS];
    uint64_t matches;  /* out: number of pairs */
    int      rc;       /* out */
    int      path;     /* out: 12, or 0 when nothing was launched */
} rhj_join_sum_desc;
int rhj_join_sum_batch_device(rhj_join_sum_desc *items, uint64_t n);

/* rhj_query_batch_device with the switch on (default off; environment RHJ_QUERY_SUM_LAST=1): a query whose LAST predicate joins
 * two nodes is, at that level, an item of one rhj_join_sum_batch_device call - the key columns and vectors of its
 * rhj_join_cols_desc, one term per view - and takes no pair buffer, no second join call and no apply item; sums and rows are
 * the same.  Everything else keeps its stages.  rhj_query_batch_last_sum_info(): the sum calls and their items of the last
 * rhj_query_batch_device (all zero with the switch off); with the switch on rhj_query_batch_info counts the pair-list calls
 * only, and an apply call only for a level where some active query is not a sum item. */
void rhj_set_query_sum_last(int on);
typedef struct rhj_query_batch_sum_info { uint32_t sum_calls, sum_items; } rhj_query_batch_sum_info;
const rhj_query_batch_sum_info *rhj_query_batch_last_sum_info(void);

/* Many weighted join folds in one call (csrc/rhj_join_fold_batch.hip.h): the primitive that sums a query whose join predicates
 * form a tree over its bindings without any intermediate result.  One item folds a child side S into a parent side R over
 * keyR(i) == keyS(j), the keys read as rhj_join_sum_desc reads them (d_col[d_sel ? d_sel[p] : p]).  A factor stands for
 *     f(p) = (d_w ? d_w[p] : 1) * (d_col ? d_col[d_src ? d_src[p] : p] : 1)          (mod 2^64, p the row's position in its side)
 * The item has nvalues child values V_c, factors over S's positions, and nouts outputs, each a value index c and a factor P
 * over R's positions:
 *     A_c(k)      = sum of V_c(j) over the rows j of S with keyS(j) == k
 *     d_out[i]    = P(i) * A_c(keyR(i))      for i < nR, when d_out is given; 0 where R's key is not in S (written, not left)
 *     total       = sum over i of P(i) * A_c(keyR(i))
 * everything exact modulo 2^64.  With every d_w NULL, a value and an output that are plain ones (d_col NULL too) give
 * rhj_join_sum_batch_device's matches as the total, and an output {NULL, d_src, d_col} on that value its side-0 sum.
 *
 * Every item with two non-empty sides runs in the launches of its chunk (path 13): one memset of the chunk's tables, at most
 * three launches (claim R's keys where R builds, add S's values, apply over R) and one stream synchronisation per chunk of at
 * most 4096 items, 2^24 tiles of 2048 rows (both sides' together) and 1 GiB of tables (8 * (1 + nvalues) bytes a slot, the
 * smallest power of two of slots that is at least twice the smaller side's rows; the smaller side claims the slots, R on a
 * tie), in call order; a chunk takes its first item whatever that needs.  Every pointer needs 8-byte alignment and no more;
 * inputs may be shared between items, sides and factors; outputs must not overlap each other or any input of the call; nothing
 * at or beyond d_out[nR] is written; the caller guarantees that every index indexes its array.  An item with an empty side has
 * rc 0, every total 0 and path 0, its d_outs are untouched and it launches nothing; a batch of 0 items returns 0 without
 * touching a device.
 *
 * The whole batch is validated before anything is launched: a NULL key column with a non-zero size, nvalues outside
 * 0..RHJ_FOLD_MAX_VALUES, nouts outside 0..RHJ_FOLD_MAX_OUTS, an output whose value index is outside 0..nvalues - 1, or a side
 * of 2^32 rows or more give that item rc -3; then nothing runs, no total is written and the call returns -3.  Otherwise 0, or a
 * negative value on a HIP error.  rhj_last_stats() afterwards: n_r and n_s the rows summed over the items, units the items
 * launched, ms_total the whole call (timing level >= 1), reserved 13. */
#define RHJ_FOLD_MAX_VALUES 9
#define RHJ_FOLD_MAX_OUTS   9
typedef struct rhj_fold_factor {
    const uint64_t *d_w;     /* NULL: 1 */
    const uint64_t *d_src;   /* NULL: q = p */
    const uint64_t *d_col;   /* NULL: 1 (d_src is not read then) */
} rhj_fold_factor;
typedef struct rhj_fold_out {
    rhj_fold_factor p;       /* over R's positions */
    uint64_t       *d_out;   /* nR words, or NULL: the total only */
    uint64_t        total;   /* out */
    int             value;   /* 0 .. nvalues - 1 */
} rhj_fold_out;
typedef struct rhj_join_fold_desc {
    const uint64_t *d_colR, *d_selR; uint64_t nR;     /* the parent side */
    const uint64_t *d_colS, *d_selS; uint64_t nS;     /* the child side */
    int             nvalues, nouts;
    rhj_fold_factor values[RHJ_FOLD_MAX_VALUES];      /* over S's positions */
    rhj_fold_out    outs[RHJ_FOLD_MAX_OUTS];
    int rc;                  /* out */
    int path;                /* out: 13 (18 for a resident item, rhj_set_fold_resident below), or 0 when nothing was launched */
} rhj_join_fold_desc;
int rhj_join_fold_batch_device(rhj_join_fold_desc *items, uint64_t n);

/* The fold schedule of one query, a pure function that needs no device.  A query FOLDS when rhj_query_levels accepts it,
 * njoins >= 1 and every step's kind is 0: each predicate joins two distinct nodes, so the predicates are a spanning tree of the
 * bindings.  Returns the number of steps (njoins = nrels - 1), 0 for a valid query that does not fold, or -3 (as
 * rhj_query_levels).  For a folding query *root is the root binding and steps[0 .. njoins) (room for RHJ_QUERY_MAX_RELS - 1) are
 * the folds, ascending by round, then by child.  The rule: the tree is rooted; a child is folded into its parent only after all
 * of its own children, in a later round than the last of them; a parent takes one child per round, among several ready children
 * the lowest binding first; every fold happens in the first round these allow.  The root is the binding that gives the fewest
 * rounds, on a tie the lowest binding.  root and steps may be NULL. */
typedef struct rhj_fold_step { int child, parent, round; } rhj_fold_step;
int rhj_query_fold_plan(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, int *root, rhj_fold_step *steps);

/* rhj_query_batch_device with the switch on (default off; environment RHJ_QUERY_FOLD=1): the filter batch runs as always; then
 * the folding queries still alive (every binding below 2^32 rows) run round by round, all of them together, each round ONE
 * rhj_join_fold_batch_device call, before the level loop of the others.  A binding carries its filter's hit list, a weight
 * vector (the rows of its folded subtree's join that each row meets) and one vector per view of that subtree (the partial view
 * sum per row); in the root's last fold nothing is written and the totals are rows and sums.  A weight total of 0 finishes the
 * query with rows = 0 and sums 0.  Folding queries take no pair buffer, no second join call, no apply item and no sum item,
 * whatever rhj_set_query_sum_last says; the other queries keep their stages and that switch.  sums are the same; rows is exact
 * MODULO 2^64: the pair route could never exceed memory, this one can exceed 2^64 (eight bindings of 2^31 rows on one key).
 * rhj_query_batch_last_fold_info(): the fold calls, their items and the queries that folded, of the last
 * rhj_query_batch_device (all zero with the switch off); with the switch on rhj_query_batch_info counts the calls and levels of
 * the other queries only (the one filter call serves all). */
void rhj_set_query_fold(int on);
typedef struct rhj_query_batch_fold_info { uint32_t fold_calls, fold_items, fold_queries; } rhj_query_batch_fold_info;
const rhj_query_batch_fold_info *rhj_query_batch_last_fold_info(void);

/* rhj_join_fold_batch_device on TUPLE keys (csrc/rhj_join_foldk_batch.hip.h): an item is rhj_join_fold_desc's with nkeys key
 * columns a side, 1 .. RHJ_FOLD_MAX_KEYS, all of a side read through its one d_sel, and keyR(i) == keyS(j) is the equality of all
 * nkeys words, word t of R against word t of S.  Values, outputs, totals and everything about chunks, tables (8 * (1 + nvalues)
 * bytes a slot), alignment, overlap and empty sides are as there; the path is 14.  No key value is special.  A slot's first word
 * holds the position of the build side's row that claimed it (and hash bits), not a key: whoever meets a taken slot compares its
 * words with that row's, read from the build side's own columns.
 *
 * Validation as for the fold batch; in addition nkeys outside 1..RHJ_FOLD_MAX_KEYS, or a NULL column among the first nkeys of a
 * side with rows, gives that item rc -3 before anything runs.  rhj_last_stats() afterwards as there, reserved 14. */
#define RHJ_FOLD_MAX_KEYS 4
typedef struct rhj_join_foldk_desc {
    int             nkeys;                             /* 1 .. RHJ_FOLD_MAX_KEYS */
    const uint64_t *d_colR[RHJ_FOLD_MAX_KEYS], *d_selR; uint64_t nR;     /* the parent side */
    const uint64_t *d_colS[RHJ_FOLD_MAX_KEYS], *d_selS; uint64_t nS;     /* the child side */
    int             nvalues, nouts;
    rhj_fold_factor values[RHJ_FOLD_MAX_VALUES];      /* over S's positions */
    rhj_fold_out    outs[RHJ_FOLD_MAX_OUTS];
    int rc;                  /* out */
    int path;                /* out: 14 (19 for a resident item, rhj_set_fold_resident_keys below), or 0 when nothing was launched */
} rhj_join_foldk_desc;
int rhj_join_foldk_batch_device(rhj_join_foldk_desc *items, uint64_t n);

/* The fold schedule of one query with its parallel predicates grouped, a pure function that needs no device.  The rule:
 * rhj_query_levels must accept the query (else -3) and njoins >= 1; a predicate whose two sides are the same binding gives 0; a
 * predicate that equals an earlier one, the same two (binding, column) terms written either way round, is dropped; the rest are
 * grouped by unordered binding pair; a group of more than RHJ_FOLD_MAX_KEYS gives 0; the groups must be exactly nrels - 1 (they
 * connect all bindings then: a spanning tree), else 0.  Schedule and root are rhj_query_fold_plan's over the groups.  A step's
 * joins[0 .. nkeys) are the indices into q->joins of its kept predicates, ascending; key word t of the parent is predicate
 * joins[t]'s column on the parent's binding, of the child its column on the child's, whichever way round it was written.  Returns
 * nrels - 1, 0 or -3.  For every query rhj_query_fold_plan accepts the root and every step's child, parent and round are the same
 * and nkeys is 1.  root and steps (room for RHJ_QUERY_MAX_RELS - 1) may be NULL. */
typedef struct rhj_foldk_step { int child, parent, round, nkeys; int joins[RHJ_FOLD_MAX_KEYS]; } rhj_foldk_step;
int rhj_query_foldk_plan(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, int *root, rhj_foldk_step *steps);

/* rhj_query_batch_device with this switch on as well as rhj_set_query_fold (default off; environment RHJ_QUERY_FOLD_KEYS=1; no
 * effect while the fold route is off): a query folds when rhj_query_foldk_plan > 0.  In a round the items with one key are ONE
 * rhj_join_fold_batch_device call, exactly as with the switch off, and the items with two or more keys ONE
 * rhj_join_foldk_batch_device call: at most two calls a round.  A binding's state, a fold's values and outputs, the round
 * buffers, the zero-total exit and the 2^64 limit are the fold route's.  rhj_query_batch_last_foldk_info(): the tuple-key calls
 * and their items, and the queries that fold only because of this switch and were alive after the filters (all zero with either
 * switch off); rhj_query_batch_fold_info keeps counting the single-key calls and items, and all folding queries. */
void rhj_set_query_fold_keys(int on);
typedef struct rhj_query_batch_foldk_info { uint32_t foldk_calls, foldk_items, foldk_queries; } rhj_query_batch_foldk_info;
const rhj_query_batch_foldk_info *rhj_query_batch_last_foldk_info(void);

/* Many folds with NO child in one call (csrc/rhj_fold_self_batch.hip.h): what a predicate with both sides on one binding, and a
 * query without a join, need on the fold route.  One item is ONE side of n rows, nterms equalities and nouts outputs, each a
 * factor P (rhj_fold_factor) over the side's positions:
 *     m(i)     = product over t of [ d_colA_t[d_selA_t ? d_selA_t[i] : i] == d_colB_t[d_selB_t ? d_selB_t[i] : i] ]   (no term: 1)
 *     d_out[i] = m(i) * P(i)       for i < n, when d_out is given; a masked row stores 0 (written, not left)
 *     total    = sum over i of m(i) * P(i)
 * everything exact modulo 2^64.  A term carries a row-id vector PER COLUMN, as rhj_filter_eq2_batch_device does: the same vector
 * twice is the predicate on one binding, two vectors the equality inside a materialised node.  A zero-term item with an output
 * {NULL, d_src, d_col} gives rhj_apply_batch_device's view sum on the same pointers as its total.
 *
 * Every item with rows runs in the ONE launch of its chunk (path 15) over 2048-row tiles: one upload, one launch, one copy of the
 * accumulator words and one stream synchronisation per chunk of at most 4096 items and 2^24 tiles, in call order.  There is no
 * table and no memset.  Every pointer needs 8-byte alignment and no more; inputs may be shared between items, terms and factors;
 * outputs must not overlap each other or any input of the call; nothing at or beyond d_out[n] is written; the caller guarantees
 * that every index indexes its array.  An item with n == 0 has rc 0, every total 0 and path 0, its d_outs are untouched and it
 * launches nothing; a batch of 0 items returns 0 without touching a device.
 *
 * The whole batch is validated before anything is launched: nterms outside 0..RHJ_FOLD_SELF_MAX_TERMS, nouts outside
 * 0..RHJ_FOLD_MAX_OUTS, a NULL column in a term of an item with rows, or n of 2^32 or more give that item rc -3; then nothing
 * runs, no total is written and the call returns -3.  Otherwise 0, or a negative value on a HIP error.  rhj_last_stats()
 * afterwards: n_r the rows summed over the items, units the items launched, ms_total the whole call (timing level >= 1),
 * reserved 15. */
#define RHJ_FOLD_SELF_MAX_TERMS 4
typedef struct rhj_fold_eq_term {
    const uint64_t *d_colA, *d_selA;   /* sel NULL: q = p */
    const uint64_t *d_colB, *d_selB;
} rhj_fold_eq_term;
typedef struct rhj_fold_self_out {
    rhj_fold_factor p;       /* over the side's positions */
    uint64_t       *d_out;   /* n words, or NULL: the total only */
    uint64_t        total;   /* out */
} rhj_fold_self_out;
typedef struct rhj_fold_self_desc {
    uint64_t          n;
    int               nterms, nouts;   /* 0 .. RHJ_FOLD_SELF_MAX_TERMS, 0 .. RHJ_FOLD_MAX_OUTS */
    rhj_fold_eq_term  terms[RHJ_FOLD_SELF_MAX_TERMS];
    rhj_fold_self_out outs[RHJ_FOLD_MAX_OUTS];
    int rc;                  /* out */
    int path;                /* out: 15, or 0 when nothing was launched */
} rhj_fold_self_desc;
int rhj_fold_self_batch_device(rhj_fold_self_desc *items, uint64_t n);

/* The fold schedule of one query with every predicate that forms no real cycle taken in, a pure function that needs no device.
 * The rule: rhj_query_levels must accept the query (else -3).  The predicates are taken in the order given over a union-find of
 * their (binding, column) terms: a predicate whose two terms are already in one class is DROPPED (the literal repeat, 0.1=0.1,
 * and the predicate that earlier ones imply: 0.1=2.1 after 0.1=1.0 and 1.0=2.1); any other is kept and joins the two classes.  A
 * kept predicate on one binding goes to self[0 .. nself), indices into q->joins, ascending; more than
 * RHJ_FOLD_SELF_MAX_TERMS of them on one binding give 0.  The other kept predicates are grouped by unordered binding pair; a group
 * of more than RHJ_FOLD_MAX_KEYS gives 0; the groups must number nrels - 1 (a spanning tree), else 0: a true cycle.  Schedule and
 * root are rhj_query_fold_plan's over one predicate per group; steps[0 .. nsteps) are as rhj_query_foldk_plan's.  A query of one
 * binding folds with nsteps 0 and root 0.  Returns 1 when the query folds, 0 when it does not, or -3.
 *
 * For every query rhj_query_foldk_plan accepts nself is 0 and the root and every step's child, parent and round are the same;
 * nkeys and joins are the same too unless a dropped predicate was implied without being a repeat (that plan keeps it as a key
 * word, this one does not).  plan may be NULL. */
typedef struct rhj_folds_plan {
    int root, nsteps, nself;
    rhj_foldk_step steps[RHJ_QUERY_MAX_RELS - 1];
    int self[RHJ_QUERY_MAX_RELS * RHJ_FOLD_SELF_MAX_TERMS];
} rhj_folds_plan;
int rhj_query_folds_plan(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, rhj_folds_plan *plan);

/* rhj_query_batch_device with this switch on as well as rhj_set_query_fold (default off; environment RHJ_QUERY_FOLD_SELF=1; no
 * effect while the fold route is off): a query that neither rhj_query_fold_plan nor (with its switch) rhj_query_foldk_plan takes
 * folds when rhj_query_folds_plan gives 1 and every step has one key or rhj_set_query_fold_keys is on.  After the filter batch
 * ONE rhj_fold_self_batch_device call runs before round 0, over all such queries still alive.  A binding with kept one-binding
 * predicates is an item of its rows, both row-id vectors of every term its hit list, and one output {ones, its first weight
 * vector}; the total is the surviving rows (below 2^32, so 0 means empty exactly) and a total of 0 finishes the query with
 * rows = 0 and sums 0.  A query of one binding is one item with every d_out NULL, output 0 {ones} its rows and one output
 * {NULL, hit list, column} per view its sums, and finishes there, with or without terms.  Then the rounds run as always, a
 * binding's weight starting at that vector instead of ones: at most two calls a round, and a binding's state, the round buffers,
 * the zero-total exit and the 2^64 limit are the fold route's.  The first weight vectors have a workspace buffer of their own.
 * rhj_query_batch_last_fold_self_info(): whether that call ran, its items, and the queries that fold only because of this switch
 * and were alive after the filters (all zero with either switch off); rhj_query_batch_fold_info keeps counting all folding
 * queries, rhj_query_batch_foldk_info the tuple-key calls and items. */
void rhj_set_query_fold_self(int on);
typedef struct rhj_query_batch_fold_self_info { uint32_t self_calls, self_items, self_queries; } rhj_query_batch_fold_self_info;
const rhj_query_batch_fold_self_info *rhj_query_batch_last_fold_self_info(void);

/* rhj_join_foldk_batch_device with a row-id vector PER KEY WORD (csrc/rhj_join_foldn_batch.hip.h): what the key of a
 * materialised node needs, whose words belong to different member bindings, each behind its own vector over the node's rows
 * (DESIGN.md 4.18).  Word t of R's row at position p is d_colR[t][d_selR[t] ? d_selR[t][p] : p], of S's likewise, t < nkeys; nR
 * and nS are the sides' positions.  Everything else is rhj_join_foldk_desc's: values, outputs and totals modulo 2^64, the slot
 * {owner, A_0 ...}, equality decided on the owner's gathered words (each through its own vector), the hash, which side builds,
 * chunks, tables, alignment, overlap, empty sides and validation (nkeys outside 1..RHJ_FOLD_MAX_KEYS or a NULL column among the
 * first nkeys of a side with rows gives rc -3 before anything runs; a vector may always be NULL).  An item whose words all name
 * one vector a side gives rhj_join_foldk_batch_device's outputs bit for bit.  The path is 16; rhj_last_stats() reserved 16. */
typedef struct rhj_join_foldn_desc {
    int             nkeys;                             /* 1 .. RHJ_FOLD_MAX_KEYS */
    const uint64_t *d_colR[RHJ_FOLD_MAX_KEYS], *d_selR[RHJ_FOLD_MAX_KEYS]; uint64_t nR;     /* the parent side */
    const uint64_t *d_colS[RHJ_FOLD_MAX_KEYS], *d_selS[RHJ_FOLD_MAX_KEYS]; uint64_t nS;     /* the child side */
    int             nvalues, nouts;
    rhj_fold_factor values[RHJ_FOLD_MAX_VALUES];      /* over S's positions */
    rhj_fold_out    outs[RHJ_FOLD_MAX_OUTS];
    int rc;                  /* out */
    int path;                /* out: 16 (19 for a resident item, rhj_set_fold_resident_keys below), or 0 when nothing was launched */
} rhj_join_foldn_desc;
int rhj_join_foldn_batch_device(rhj_join_foldn_desc *items, uint64_t n);

/* Where a query can hand over from levels to folds over merged nodes, a pure function that needs no device.  -3 where
 * rhj_query_levels gives it, 1 for every other query.  For a prefix L of the predicates the rule is: the first L predicates run as
 * levels, so each merges its two bindings' nodes (B's node takes A's id, as rhj_query_levels names nodes) and joins its two
 * (binding, column) terms in a union-find; the remaining predicates go through that same union-find in the order given; one whose
 * terms are in one class already is dropped; a kept one with both bindings in one node is an inside predicate of that node, and
 * more than RHJ_FOLD_SELF_MAX_TERMS of them on a node fail L; the other kept ones are grouped by unordered node pair, and a group
 * of more than RHJ_FOLD_MAX_KEYS fails L; the groups must number (nodes - 1), else L fails.  levels is the smallest L that
 * passes; it is at most max(njoins - 1, 0).  node[b] is binding b's node after those levels; root, steps[0 .. nsteps) and
 * self[0 .. nself) are rhj_folds_plan's with node ids as child, parent and root: the schedule is rhj_query_fold_plan's over the
 * nodes (fewest rounds, the lowest node id on a tie).  Key word t of a step is predicate joins[t]: the parent's word is the term
 * whose binding lies in the parent node, the child's the other.  The predicates are not reordered: a first predicate off a cycle
 * is merged like any other.  At levels 0 the plan is rhj_query_folds_plan's wherever that gives 1.  plan may be NULL. */
typedef struct rhj_foldn_plan {
    int levels, root, nsteps, nself;
    int node[RHJ_QUERY_MAX_RELS];
    rhj_foldk_step steps[RHJ_QUERY_MAX_RELS - 1];
    int self[RHJ_QUERY_MAX_RELS * RHJ_FOLD_SELF_MAX_TERMS];
} rhj_foldn_plan;
int rhj_query_foldn_plan(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, rhj_foldn_plan *plan);

/* rhj_query_batch_device with this switch on as well as rhj_set_query_fold, rhj_set_query_fold_keys and rhj_set_query_fold_self
 * (default off; environment RHJ_QUERY_FOLD_NODES=1; no effect unless all three are on): a query that none of the three plans
 * takes, whose bindings each have fewer than 2^32 rows, runs rhj_query_foldn_plan's `levels` as levels and folds over its merged
 * nodes from there.  The filter batch and the fold pass of the queries that fold from the start run as always;
 * in the level loop such a query takes part in levels 0 .. levels - 1 only (it rebuilds there and never finishes, nor takes the
 * rhj_set_query_sum_last form) and is parked; after the loop the nodes' pass runs over the parked queries still alive: ONE
 * rhj_fold_self_batch_device call (a node with inside predicates is an item over the node's rows, each term's columns through the
 * row-id vectors of the bindings it names; a query that is one node is one item with its views as outputs and finishes there),
 * then the rounds, with weights and carried views per node; a key word, a child's view value and a root's lazy view read their
 * column through the vector of the member binding named.  A round's items on one key are one rhj_join_fold_batch_device call,
 * those on several words that name ONE binding a side one rhj_join_foldk_batch_device call, those whose words name several
 * members of a side one rhj_join_foldn_batch_device call: at most three calls a round.  The zero-total exit, the 2^64 limit and
 * the round buffers are the fold route's.  A query whose merged node has rhj_set_query_fold_node_rows's limit of rows or more at
 * its hand-over (default and most 2^32; larger values clamp) stays on the levels to its end.
 * rhj_query_batch_last_fold_nodes_info(): the rhj_join_foldn_batch_device calls and their items, the queries parked alive and
 * the sum of their levels (all zero unless all four switches are on).  The fold, foldk and self infos count both passes'
 * calls and items, and fold_queries the parked queries too; rhj_query_batch_info counts the levels and calls of the level queries
 * and of the prefixes. */
void rhj_set_query_fold_nodes(int on);
void rhj_set_query_fold_node_rows(uint64_t limit);
typedef struct rhj_query_batch_fold_nodes_info { uint32_t foldn_calls, foldn_items, node_queries, node_levels; } rhj_query_batch_fold_nodes_info;
const rhj_query_batch_fold_nodes_info *rhj_query_batch_last_fold_nodes_info(void);

/* rhj_fold_self_batch_device with CONSTANT predicates in the mask (csrc/rhj_fold_pred_batch.hip.h): a filter as a 0/1 factor on a
 * side's weights, with no hit list.  One item is ONE side of n rows, nconst comparisons, neq equalities and nouts
 * outputs, each a factor P (rhj_fold_factor) over the side's positions:
 *     m(i)     = AND over c of [ d_col_c[d_sel_c ? d_sel_c[i] : i]  op_c  value_c ]  AND  over t of [ A_t == B_t ]     (no term: 1)
 *     d_out[i] = m(i) * P(i)       for i < n, when d_out is given; a masked row stores 0 (written, not left)
 *     total    = sum over i of m(i) * P(i)
 * everything exact modulo 2^64.  op is '<', '>' or '=' and the comparison is UNSIGNED, value already converted, as
 * rhj_filter_device's; the equalities are rhj_fold_self_desc's terms.  With nconst 0 an item gives rhj_fold_self_batch_device's
 * outputs bit for bit; with one output {ones} its total is rhj_filter_batch_device's hits on the same terms.
 *
 * Every item with rows runs in the ONE launch of its chunk (path 17) over 2048-row tiles: one upload, one launch, one copy of the
 * accumulator words and one stream synchronisation per chunk of at most 4096 items and 2^24 tiles, in call order.  There is no
 * table and no memset.  Pointers, sharing, overlap, d_out[n] and empty items are as there: an item with n == 0 has rc 0, every
 * total 0 and path 0, its d_outs are untouched and it launches nothing; a batch of 0 items returns 0 without touching a device.
 *
 * The whole batch is validated before anything is launched: an op outside '<', '>', '=', nconst outside
 * 0..RHJ_FILTER_MAX_TERMS, neq outside 0..RHJ_FOLD_SELF_MAX_TERMS, nouts outside 0..RHJ_FOLD_MAX_OUTS, a NULL column in a term of
 * an item with rows, or n of 2^32 or more give that item rc -3; then nothing runs, no total is written and the call returns -3.
 * Otherwise 0, or a negative value on a HIP error.  rhj_last_stats() afterwards: n_r the rows summed over the items, units the
 * items launched, ms_total the whole call (timing level >= 1), reserved 17. */
typedef struct rhj_fold_const_term {
    const uint64_t *d_col, *d_sel;     /* sel NULL: q = p */
    char            op;                /* '<', '>' or '=' */
    uint64_t        value;
} rhj_fold_const_term;
typedef struct rhj_fold_pred_desc {
    uint64_t            n;
    int                 nconst, neq, nouts;   /* 0 .. RHJ_FILTER_MAX_TERMS, 0 .. RHJ_FOLD_SELF_MAX_TERMS, 0 .. RHJ_FOLD_MAX_OUTS */
    rhj_fold_const_term consts[RHJ_FILTER_MAX_TERMS];
    rhj_fold_eq_term    eqs[RHJ_FOLD_SELF_MAX_TERMS];
    rhj_fold_self_out   outs[RHJ_FOLD_MAX_OUTS];
    int rc;                  /* out */
    int path;                /* out: 17, or 0 when nothing was launched */
} rhj_fold_pred_desc;
int rhj_fold_pred_batch_device(rhj_fold_pred_desc *items, uint64_t n);

/* rhj_query_batch_device with this switch on as well as rhj_set_query_fold (default off; environment RHJ_QUERY_FOLD_ONE_WAIT=1; no
 * effect while the fold route is off): a FOLD PROGRAM with one wait.  A query takes this route when, under the
 * fold, keys and self switches as they stand, rhj_query_fold_plan, rhj_query_foldk_plan or rhj_query_folds_plan lets it fold (a
 * query that hands over from levels, rhj_set_query_fold_nodes's, does not) and every binding's relation has between 1 row and
 * rhj_set_query_fold_one_wait_rows's limit (default 4096: the largest size at which the route measured no slower on filtered chains; `small` needs 65 536 and gains with it).  rhj_query_one_wait_plan says so of one query: 1 it takes the route,
 * 0 it is valid and does not, -3 as rhj_query_levels; a pure function that needs no device (rels may not be NULL for a 1: the
 * rule reads the rows; with rels NULL it gives 0 or -3).
 *
 * For such a query no filter item is issued: a binding's side is its WHOLE relation (no row-id vector), and its filters and kept
 * one-binding predicates are ONE rhj_fold_pred_desc item whose output {ones} is the binding's first weight vector; a query with
 * no join is one such item with its views as outputs.  Every size of every round is then known before the device is touched, so
 * the route's queries, in call order, are one program: one upload of every descriptor, tile start and zeroed accumulator word,
 * one k_fold_pred launch, per round one memset of that round's tables and the fold batches' unchanged launches on one key and on
 * tuple keys, one copy of all words back and ONE stream synchronisation.  A program is cut only where a batch's chunk would be:
 * 4096 items a round and kind (and pred items), 2^24 tiles a launch, 1 GiB of tables a round.  The answers follow the fold
 * route's rule, so the two agree bit for bit, the 2^64 limit included: a query is empty (rows 0, sums 0) when a pred item's
 * weight total or a step's first total is 0; else rows and sums are the last step's totals, or the join-less item's.  There is
 * no early exit: zero weights propagate.  The other queries run exactly as with the switch off, after the programs, and every
 * other info struct counts them alone.  rhj_query_batch_last_one_wait_info(): the route's queries, the programs, their items by
 * kind, the rounds, kernel launches, memsets and stream synchronisations summed over the programs (all zero with the switch off). */
void rhj_set_query_fold_one_wait(int on);
void rhj_set_query_fold_one_wait_rows(uint64_t limit);
int rhj_query_one_wait_plan(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels);
typedef struct rhj_query_batch_one_wait_info { uint32_t queries, programs, pred_items, fold_items, foldk_items, rounds, launches, memsets, waits; } rhj_query_batch_one_wait_info;
const rhj_query_batch_one_wait_info *rhj_query_batch_last_one_wait_info(void);

/* The components of one query, a pure function that needs no device: rhj_query_levels' validation without its last rule (all
 * bindings in one node after the last predicate).  Returns the number of components (1 where rhj_query_levels accepts the query,
 * more for a cross product, at most RHJ_QUERY_MAX_RELS), or -3 for exactly the other queries rhj_query_levels refuses.  comp[b],
 * when given, is the component of binding b; components are numbered 0, 1, ... in the order of their lowest binding.  rels may be
 * NULL as there. */
int rhj_query_components(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, int *comp);

/* rhj_query_batch_device with the switch on (default off; environment RHJ_QUERY_PRODUCTS=1): a query of k > 1 components, a
 * CROSS PRODUCT, is accepted.  The product is never built.  With T_c the rows of component c alone and S_v the
 * sum of view v over the component c(v) its binding lies in,
 *     rows    = product over c of T_c                        (mod 2^64)
 *     sums[v] = S_v * product over c != c(v) of T_c          (mod 2^64)
 * which is what wrap-around sums over CartesianInterResults' n1 * n2 * ... rows give.  The caller's batch is validated first
 * (rhj_query_components: -3 and nothing ran for what that refuses; rc is set on the caller's descriptors).  If it holds such a
 * query, the call runs an internal batch of its own in ONE pass through the stages above: every one-component query unchanged, and
 * every other query as k component queries in its place - the component's bindings renumbered 0.. in ascending order, its filters,
 * predicates and views in their order, and for a component without a view one stand-in view (the first column its first predicate
 * names, else its first filter's, else the relation's first column) whose sum is not read.  A component that is one binding with
 * no filter, no view and no column has its relation's rows and takes no place in that batch.  All components of all queries share
 * the filter batch, the levels, the fold rounds and the programs, each on the route the other switches give a query of its
 * shape; the products are taken on the host.  rows == 0 reads as empty, as everywhere: when a component is empty, or the
 * product is 0 modulo 2^64 (2^22 * 2^22 * 2^20 rows), rows and every sum are 0.  The one-component queries of such a batch get bit
 * for bit the answers of a call without the others.  A batch without a cross product runs exactly as with the switch off.
 * rhj_query_levels and the plan functions do not look at the switch: they keep -3 for a cross product.
 * rhj_query_batch_last_products_info(): the caller's queries of several components in the last rhj_query_batch_device, and
 * their components (zero with the switch off or none in the batch); every other info struct then counts the internal batch
 * (fold_queries counts components).  rhj_last_stats(): n_r the caller's queries, matches the sum of their rows, reserved 10. */
void rhj_set_query_products(int on);
typedef struct { uint32_t product_queries, components; } rhj_query_batch_products_info;
const rhj_query_batch_products_info *rhj_query_batch_last_products_info(void);

/* The four table batches with this switch on (rhj_join_sum_batch_device, rhj_join_fold_batch_device, rhj_join_foldk_batch_device,
 * rhj_join_foldn_batch_device; environment RHJ_FOLD_COMBINE=0|1; DEFAULT ON: the uniform cases measured within the spread of the
 * build before it): a WORKGROUP-LEVEL COMBINER in their add launches (csrc/rhj_slot_combine.hip.h).
 * Without it every row sends one device-scope atomic per value into the slot of its key, and one address takes about 80 adds a
 * microsecond: a side of few distinct keys costs the multiplicity of its hottest key.  With it the adds of a 2048-row tile to one
 * slot meet in LDS (2048 entries, a row's entry the low bits of its slot index; a row that finds another slot in its entry adds
 * by itself, as before) and ONE atomic per (tile, slot, value) goes to the table.  A tile with fewer than 64 rows that found
 * their slot's entry taken by their own slot adds per row, as with the switch off.  Sums modulo 2^64 and counts do not depend on
 * the order of their terms: every output vector, total, match count and sum is bit for bit the same under both settings.  The
 * switch reaches the batches wherever they are issued: the four entry points, the fold route of rhj_query_batch_device and its
 * one-wait programs.  Tables, chunks, launch counts, path ids and every struct above are as with the switch off.
 *
 * rhj_table_batch_last_combine_info(): `tiles` the add launches' tiles (a fold's child-side tiles; both count launches' of a join
 * sum), `combined_tiles` those that combined, `slot_adds` the device-scope adds into table slots that were issued (owners' sums,
 * rows that went by themselves, a non-combining tile's adds; adds of 0 are never issued, and the empty key's words are no slot).
 * Reset on entry to each of the four batches and to rhj_query_batch_device, whose inner table batches sum into it; all zero with
 * the switch off, and after a batch that was refused (-3). */
void rhj_set_fold_combine(int on);
int rhj_get_fold_combine(void);          /* the switch as it stands: the default, the environment's value or the last call's */
typedef struct {
    uint64_t tiles;           /* add-launch tiles with the switch on */
    uint64_t combined_tiles;
    uint64_t slot_adds;
} rhj_table_batch_combine_info;
const rhj_table_batch_combine_info *rhj_table_batch_last_combine_info(void);

/* rhj_join_fold_batch_device with this switch on (DEFAULT OFF; environment RHJ_FOLD_RESIDENT=0|1): an item whose
 * table fits a workgroup's LDS is RESIDENT (csrc/rhj_fold_lds.hip.h): ONE workgroup folds it in ONE launch, k_fold_lds, the table
 * in LDS.  Such an item has no table in the arena, so it counts 0 bytes where a batch is cut into chunks (its tiles and itself
 * count as ever: 4096 items and 2^24 tiles still cut), it is not part of the chunk's memset and it has no tile in the three
 * launches.  A chunk is still one upload, one copy back and one stream synchronisation; its resident items are one k_fold_lds
 * launch, if it has any, and the others the memset of their tables and the three launches, if it has any.  Every d_out word and
 * every total is bit for bit what the table form gives (sums modulo 2^64 do not depend on the order of their terms); call order
 * of the results, rc, validation, empty sides and the refusal of a whole batch are unchanged.  A resident item reports path 18;
 * rhj_last_stats().reserved of the call stays 13.  It brings no combiner counters and no tile to
 * rhj_table_batch_last_combine_info(), which counts the table items only.  The switch reaches the fold batches on one key
 * wherever they are issued: the entry point, the fold route of rhj_query_batch_device by waits, and its one-wait programs, where
 * a round whose items are all resident issues no memset and one launch (rhj_query_batch_one_wait_info counts what was issued).
 * The folds on tuple keys have a resident form under a switch of their own (rhj_set_fold_resident_keys below); the join sums have none.
 *
 * rhj_fold_resident_rule(nR, nS, nvalues), a pure function that needs no device: 1 when an item of these sizes is resident
 * while the switch is on, else 0.  All of: both sides have rows; slots * (1 + nvalues) <= 16 384 u64 words (128 KiB), slots the
 * table's rule (the smallest power of two that is at least twice the rows of the side that builds: the smaller, R on a tie); and
 * the other side, which the one workgroup walks alone, has at most 16 384 rows (both constants in csrc/rhj_fold_lds.hip.h; DESIGN.md 6 has the measurement behind the second).
 *
 * rhj_table_batch_last_resident_info(): the resident items, the k_fold_lds launches and the table items of the fold batches on
 * one key.  Reset where rhj_table_batch_last_combine_info() is; all zero with the switch off. */
void rhj_set_fold_resident(int on);
int rhj_get_fold_resident(void);         /* the switch as it stands: the default, the environment's value or the last call's */
int rhj_fold_resident_rule(uint64_t nR, uint64_t nS, int nvalues);
typedef struct { uint32_t resident_items, resident_launches, table_items; } rhj_table_batch_resident_info;
const rhj_table_batch_resident_info *rhj_table_batch_last_resident_info(void);

/* rhj_join_foldk_batch_device and rhj_join_foldn_batch_device with this switch on (DEFAULT OFF; environment
 * RHJ_FOLD_RESIDENT_KEYS=0|1): the resident form above for the folds on tuple keys
 * (csrc/rhj_fold_keys_lds.hip.h).  ONE workgroup folds a resident item in ONE launch, k_foldk_lds or k_foldn_lds.  The table in
 * LDS is the table of the arena: a slot holds the build row that owns it and the sums, not the key, and equality is still
 * decided on the owner's words, gathered from the build side's columns in memory.  Such an item counts 0 bytes where a batch is
 * cut into chunks (4096 items and 2^24 tiles still cut), is not part of the chunk's memset and has no tile in the three
 * launches; a chunk whose items are all resident issues no memset and one launch, a mixed one the memset and three launches of
 * its table items and then the resident launch.  Every d_out word and every total is bit for bit what the table form gives;
 * call order, rc, validation, empty sides and the refusal of a whole batch are unchanged.  A resident item reports path 19;
 * rhj_last_stats().reserved of the call stays 14 or 16.  The switch is independent of rhj_set_fold_resident: with that one
 * alone the items on tuple keys keep paths 14 and 16, with this one alone the items on one key keep 13.  It reaches the
 * tuple-key folds wherever they are issued: the two entry points, the fold route of rhj_query_batch_device by waits, and its
 * one-wait programs, where a round's items on tuple keys have a resident launch of their own behind their table launches (which
 * run only if a table item exists); with both switches on, a round whose items are all resident issues no memset and at most
 * two launches.
 *
 * rhj_fold_resident_keys_rule(nR, nS, nvalues), a pure function that needs no device: 1 when an item of these sizes is resident
 * while the switch is on, else 0.  All of: both sides have rows; 0 <= nvalues <= 9; slots * (1 + nvalues) <= 16 384 u64 words,
 * slots the table's rule; and the other side has at most 4096 rows (FOLDK_LDS_MAX_ROWS in csrc/rhj_fold_keys_lds.hip.h;
 * DESIGN.md 6 has the measurement behind it).  The number of key columns does not enter: a slot holds an owner, not a key.
 *
 * rhj_table_batch_last_resident_keys_info(): the resident items, the k_foldk_lds and k_foldn_lds launches and the table items of
 * the two batches on tuple keys.  Reset where rhj_table_batch_last_resident_info() is; all zero with the switch off. */
void rhj_set_fold_resident_keys(int on);
int rhj_get_fold_resident_keys(void);    /* the switch as it stands: the default, the environment's value or the last call's */
int rhj_fold_resident_keys_rule(uint64_t nR, uint64_t nS, int nvalues);
const rhj_table_batch_resident_info *rhj_table_batch_last_resident_keys_info(void);

/* 1 when the object was created by this library's device-resident side */
int rhj_resident_relation(const rhj_relation *rel);
int rhj_resident_result(const rhj_result *res);
int rhj_resident_inter(const rhj_inter_res *head);

#ifdef __cplusplus
}
#endif
#endif /* RHJ_INTER_H */
