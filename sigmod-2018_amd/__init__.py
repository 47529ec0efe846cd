"""sigmod-2018_amd — MI355X-native radix hash join / filter scan behind the C-ABI of
include/rhj.h (librhj.so: hand-written gfx950 kernels + the reference's own C entry
points RadixHashJoin()/Filter()).

This module is a thin ctypes binding used by tests/ and bench.py; PyTorch supplies
device memory and streams only.  There is no CPU path: loading fails loudly when
librhj.so is missing, and every call fails when no GPU is visible.

Import with importlib (the directory name carries a hyphen):
    rhj = importlib.import_module("sigmod-2018_amd")
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "librhj.so")

TUPLE = np.dtype([("value", "<u8"), ("row_id", "<u8")])       # structs.h:15-19
PAIR = np.dtype([("row_idR", "<u8"), ("row_idS", "<u8")])     # structs.h:46-50

# every symbol include/rhj.h declares; tests check the library exports all of them
ABI_SYMBOLS = [
    "RadixHashJoin", "Filter", "InsertResult", "InsertRowIdResult", "GetResultNum", "FindResultRowId",
    "FindResultTuples", "FreeResult", "PrintResult", "FreeRelation", "SchedulerInit", "SchedulerDestroy",
    "rhj_set_radix_bits", "rhj_get_radix_bits", "rhj_set_empty_mode", "rhj_set_node_pairs", "rhj_set_device", "rhj_get_device",
    "rhj_set_stream", "rhj_set_force_hbm_table", "rhj_set_fused", "rhj_set_resident", "rhj_set_small", "rhj_set_lowradix", "rhj_set_count_in_pass1", "rhj_set_spec", "rhj_last_spec", "rhj_set_exact", "rhj_last_exact", "rhj_set_walk_count", "rhj_last_walk_units", "rhj_set_devices", "rhj_get_devices", "rhj_device_range", "rhj_set_devices_balance", "rhj_plan_device_ranges", "rhj_plan_device_slices", "rhj_cut_to_slice", "rhj_join_devices", "rhj_gather_pairs_devices", "rhj_set_order", "rhj_get_order", "rhj_auto_radix_bits", "rhj_sub_bits", "rhj_set_timing", "rhj_join_device", "rhj_join_batch_device", "rhj_batch_takes", "rhj_join_cols_batch_device", "rhj_join_cols_device", "rhj_join_keys_device", "rhj_partition_device", "rhj_filter_device", "rhj_filter_batch_device", "rhj_filter_batch_takes",
    "rhj_register_relation_map", "rhj_unregister_relation_map", "rhj_registered_columns", "rhj_pinned_ranges",
    "rhj_bucket_histogram_device", "rhj_select_bucket_range_device", "rhj_join_device_range", "rhj_join_device_slice", "rhj_pin_refusals",
    "rhj_release", "rhj_last_stats", "rhj_version",
]
# every symbol include/rhj_inter.h declares (device-resident intermediate results)
INTER_SYMBOLS = [
    "InitInterData", "FreeInterData", "InitInterResults", "PrintInterResults", "FreeInterResults",
    "InsertJoinToInterResults", "GetRelation", "ScanInterResults", "SelfJoin", "MergeInterNodes", "Merge",
    "CalculateQueryResults", "PrintNullResults", "AreActiveInInter", "JoinInterNode", "CartesianInterResults",
    "InsertSingleRowIdsToInterResult", "rhj_gather_tables_device", "rhj_build_relation_device", "rhj_sum_gather_device", "rhj_sum_views_device",
    "rhj_filter_eq2_device", "rhj_resident_relation", "rhj_resident_result", "rhj_resident_inter",
    "InitRelationMap", "FreeRelationMap", "PrintRelationMap", "rhj_column_stats_device", "rhj_apply_batch_device",
    "rhj_filter_eq2_batch_device", "rhj_query_batch_device", "rhj_query_levels", "rhj_query_batch_last_info",
    "rhj_column_stats_batch_device", "rhj_column_stats_flags", "rhj_column_stats_batch_last_info",
    "rhj_join_sum_batch_device", "rhj_set_query_sum_last", "rhj_query_batch_last_sum_info",
    "rhj_join_fold_batch_device", "rhj_query_fold_plan", "rhj_set_query_fold", "rhj_query_batch_last_fold_info",
    "rhj_join_foldk_batch_device", "rhj_query_foldk_plan", "rhj_set_query_fold_keys", "rhj_query_batch_last_foldk_info",
    "rhj_fold_self_batch_device", "rhj_query_folds_plan", "rhj_set_query_fold_self", "rhj_query_batch_last_fold_self_info",
    "rhj_join_foldn_batch_device", "rhj_query_foldn_plan", "rhj_set_query_fold_nodes", "rhj_set_query_fold_node_rows", "rhj_query_batch_last_fold_nodes_info",
    "rhj_fold_pred_batch_device", "rhj_query_one_wait_plan", "rhj_set_query_fold_one_wait", "rhj_set_query_fold_one_wait_rows", "rhj_query_batch_last_one_wait_info",
    "rhj_query_components", "rhj_set_query_products", "rhj_query_batch_last_products_info",
    "rhj_set_fold_combine", "rhj_get_fold_combine", "rhj_table_batch_last_combine_info",
    "rhj_set_fold_resident", "rhj_get_fold_resident", "rhj_fold_resident_rule", "rhj_table_batch_last_resident_info",
    "rhj_set_fold_resident_keys", "rhj_get_fold_resident_keys", "rhj_fold_resident_keys_rule", "rhj_table_batch_last_resident_keys_info",
]


class Relation(C.Structure):
    _fields_ = [("tuples", C.c_void_p), ("num_tuples", C.c_uint64)]


class Result(C.Structure):
    pass


Result._fields_ = [("buff", C.c_void_p), ("next", C.POINTER(Result)), ("current_load", C.c_uint64)]


class InterData(C.Structure):
    _fields_ = [("num_tuples", C.c_uint64), ("table", C.POINTER(C.c_void_p))]


class InterRes(C.Structure):
    pass


InterRes._fields_ = [("data", C.POINTER(InterData)), ("num_of_relations", C.c_int), ("next", C.POINTER(InterRes))]


class ColumnStats(C.Structure):
    _fields_ = [("l", C.c_uint64), ("u", C.c_uint64), ("f", C.c_double), ("d", C.c_double)]


class RelationMap(C.Structure):
    _fields_ = [("num_tuples", C.c_uint64), ("num_columns", C.c_uint64), ("columns", C.POINTER(C.c_void_p)),
                ("col_stats", C.POINTER(ColumnStats))]


class FilterPred(C.Structure):
    _fields_ = [("relation", C.c_int), ("column", C.c_int), ("value", C.c_int), ("comperator", C.c_char)]


class JoinDesc(C.Structure):
    """rhj_join_desc (include/rhj.h): one join of rhj_join_batch_device"""
    _fields_ = [("d_R", C.c_void_p), ("nR", C.c_uint64), ("d_S", C.c_void_p), ("nS", C.c_uint64),
                ("d_out", C.c_void_p), ("out_capacity", C.c_uint64), ("matches", C.c_uint64), ("rc", C.c_int), ("path", C.c_int)]


class JoinColsDesc(C.Structure):
    """rhj_join_cols_desc (include/rhj.h): one join of rhj_join_cols_batch_device"""
    _fields_ = [("d_colR", C.c_void_p), ("d_selR", C.c_void_p), ("nR", C.c_uint64),
                ("d_colS", C.c_void_p), ("d_selS", C.c_void_p), ("nS", C.c_uint64),
                ("d_out", C.c_void_p), ("out_capacity", C.c_uint64), ("matches", C.c_uint64), ("rc", C.c_int), ("path", C.c_int)]


FILTER_MAX_TERMS = 4                     # RHJ_FILTER_MAX_TERMS


class FilterTerm(C.Structure):
    """rhj_filter_term (include/rhj.h): one predicate of a batched filter"""
    _fields_ = [("d_col", C.c_void_p), ("value", C.c_uint64), ("op", C.c_char)]


class FilterDesc(C.Structure):
    """rhj_filter_desc (include/rhj.h): one filter of rhj_filter_batch_device"""
    _fields_ = [("d_sel", C.c_void_p), ("n", C.c_uint64), ("nterms", C.c_int), ("terms", FilterTerm * FILTER_MAX_TERMS),
                ("d_out", C.c_void_p), ("hits", C.c_uint64), ("rc", C.c_int), ("path", C.c_int)]


APPLY_MAX_TERMS = 8                      # RHJ_APPLY_MAX_TERMS


class ApplyTerm(C.Structure):
    """rhj_apply_term (include/rhj_inter.h): one term of a batched apply item"""
    _fields_ = [("d_src", C.c_void_p), ("d_dst", C.c_void_p), ("d_col", C.c_void_p), ("sum", C.c_uint64), ("side", C.c_int)]


class ApplyDesc(C.Structure):
    """rhj_apply_desc (include/rhj_inter.h): one item of rhj_apply_batch_device"""
    _fields_ = [("d_idx", C.c_void_p), ("n", C.c_uint64), ("idx_stride", C.c_int), ("nterms", C.c_int),
                ("terms", ApplyTerm * APPLY_MAX_TERMS), ("rc", C.c_int), ("path", C.c_int)]


class Eq2Desc(C.Structure):
    """rhj_eq2_desc (include/rhj_inter.h): one item of rhj_filter_eq2_batch_device"""
    _fields_ = [("d_colA", C.c_void_p), ("d_selA", C.c_void_p), ("d_colB", C.c_void_p), ("d_selB", C.c_void_p), ("n", C.c_uint64),
                ("d_out", C.c_void_p), ("hits", C.c_uint64), ("rc", C.c_int), ("path", C.c_int)]


QUERY_MAX_RELS = 8                       # RHJ_QUERY_MAX_RELS
QUERY_MAX_VIEWS = 8                      # RHJ_QUERY_MAX_VIEWS


class DeviceRelation(C.Structure):
    """rhj_device_relation (include/rhj_inter.h): a device-resident column store"""
    _fields_ = [("num_tuples", C.c_uint64), ("num_columns", C.c_uint64), ("d_columns", C.POINTER(C.c_void_p))]


class QueryFilter(C.Structure):
    _fields_ = [("rel", C.c_int), ("col", C.c_int), ("op", C.c_char), ("value", C.c_uint64)]


class QueryJoin(C.Structure):
    _fields_ = [("relA", C.c_int), ("colA", C.c_int), ("relB", C.c_int), ("colB", C.c_int)]


class QueryView(C.Structure):
    _fields_ = [("rel", C.c_int), ("col", C.c_int)]


class QueryDesc(C.Structure):
    """rhj_query_desc (include/rhj_inter.h): one query of rhj_query_batch_device"""
    _fields_ = [("nrels", C.c_int), ("rels", C.POINTER(C.c_int)), ("nfilters", C.c_int), ("filters", C.POINTER(QueryFilter)),
                ("njoins", C.c_int), ("joins", C.POINTER(QueryJoin)), ("nviews", C.c_int), ("views", C.POINTER(QueryView)),
                ("sums", C.c_uint64 * QUERY_MAX_VIEWS), ("rows", C.c_uint64), ("rc", C.c_int)]


class QueryBatchInfo(C.Structure):
    """rhj_query_batch_info (include/rhj_inter.h): the calls the last rhj_query_batch_device issued"""
    _fields_ = [(n, C.c_uint32) for n in ("levels", "filter_calls", "eq2_calls", "join_calls", "join_reruns", "apply_calls")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ColStatsDesc(C.Structure):
    """rhj_colstats_desc (include/rhj_inter.h): one column of rhj_column_stats_batch_device"""
    _fields_ = [("d_col", C.c_void_p), ("n", C.c_uint64), ("l", C.c_uint64), ("u", C.c_uint64), ("d", C.c_double),
                ("rc", C.c_int), ("path", C.c_int)]


class ColStatsBatchInfo(C.Structure):
    """rhj_colstats_batch_info (include/rhj_inter.h): what the last rhj_column_stats_batch_device ran"""
    _fields_ = [("chunks", C.c_uint32), ("columns", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


JOIN_SUM_MAX_TERMS = 8                   # RHJ_JOIN_SUM_MAX_TERMS


class JoinSumTerm(C.Structure):
    """rhj_join_sum_term (include/rhj_inter.h): one term of a batched join-sum item"""
    _fields_ = [("d_src", C.c_void_p), ("d_col", C.c_void_p), ("sum", C.c_uint64), ("side", C.c_int)]


class JoinSumDesc(C.Structure):
    """rhj_join_sum_desc (include/rhj_inter.h): one item of rhj_join_sum_batch_device"""
    _fields_ = [("d_colR", C.c_void_p), ("d_selR", C.c_void_p), ("nR", C.c_uint64),
                ("d_colS", C.c_void_p), ("d_selS", C.c_void_p), ("nS", C.c_uint64),
                ("nterms", C.c_int), ("terms", JoinSumTerm * JOIN_SUM_MAX_TERMS),
                ("matches", C.c_uint64), ("rc", C.c_int), ("path", C.c_int)]


class QueryBatchSumInfo(C.Structure):
    """rhj_query_batch_sum_info (include/rhj_inter.h): the sum calls the last rhj_query_batch_device issued, and their items"""
    _fields_ = [("sum_calls", C.c_uint32), ("sum_items", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


FOLD_MAX_VALUES = 9                      # RHJ_FOLD_MAX_VALUES
FOLD_MAX_OUTS = 9                        # RHJ_FOLD_MAX_OUTS


class FoldFactor(C.Structure):
    """rhj_fold_factor (include/rhj_inter.h): f(p) = (d_w ? d_w[p] : 1) * (d_col ? d_col[d_src ? d_src[p] : p] : 1)"""
    _fields_ = [("d_w", C.c_void_p), ("d_src", C.c_void_p), ("d_col", C.c_void_p)]


class FoldOut(C.Structure):
    """rhj_fold_out (include/rhj_inter.h): one output of a batched join-fold item"""
    _fields_ = [("p", FoldFactor), ("d_out", C.c_void_p), ("total", C.c_uint64), ("value", C.c_int)]


class JoinFoldDesc(C.Structure):
    """rhj_join_fold_desc (include/rhj_inter.h): one item of rhj_join_fold_batch_device"""
    _fields_ = [("d_colR", C.c_void_p), ("d_selR", C.c_void_p), ("nR", C.c_uint64),
                ("d_colS", C.c_void_p), ("d_selS", C.c_void_p), ("nS", C.c_uint64),
                ("nvalues", C.c_int), ("nouts", C.c_int),
                ("values", FoldFactor * FOLD_MAX_VALUES), ("outs", FoldOut * FOLD_MAX_OUTS),
                ("rc", C.c_int), ("path", C.c_int)]


class FoldStep(C.Structure):
    """rhj_fold_step (include/rhj_inter.h): one fold of rhj_query_fold_plan's schedule"""
    _fields_ = [("child", C.c_int), ("parent", C.c_int), ("round", C.c_int)]


class QueryBatchFoldInfo(C.Structure):
    """rhj_query_batch_fold_info (include/rhj_inter.h): the fold calls the last rhj_query_batch_device issued, their items and the
    queries that went through them"""
    _fields_ = [("fold_calls", C.c_uint32), ("fold_items", C.c_uint32), ("fold_queries", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


FOLD_MAX_KEYS = 4                        # RHJ_FOLD_MAX_KEYS


class JoinFoldKDesc(C.Structure):
    """rhj_join_foldk_desc (include/rhj_inter.h): one item of rhj_join_foldk_batch_device"""
    _fields_ = [("nkeys", C.c_int),
                ("d_colR", C.c_void_p * FOLD_MAX_KEYS), ("d_selR", C.c_void_p), ("nR", C.c_uint64),
                ("d_colS", C.c_void_p * FOLD_MAX_KEYS), ("d_selS", C.c_void_p), ("nS", C.c_uint64),
                ("nvalues", C.c_int), ("nouts", C.c_int),
                ("values", FoldFactor * FOLD_MAX_VALUES), ("outs", FoldOut * FOLD_MAX_OUTS),
                ("rc", C.c_int), ("path", C.c_int)]


class FoldKStep(C.Structure):
    """rhj_foldk_step (include/rhj_inter.h): one fold of rhj_query_foldk_plan's schedule"""
    _fields_ = [("child", C.c_int), ("parent", C.c_int), ("round", C.c_int), ("nkeys", C.c_int), ("joins", C.c_int * FOLD_MAX_KEYS)]


class QueryBatchFoldKInfo(C.Structure):
    """rhj_query_batch_foldk_info (include/rhj_inter.h): the tuple-key fold calls the last rhj_query_batch_device issued, their
    items and the queries that folded only because of rhj_set_query_fold_keys"""
    _fields_ = [("foldk_calls", C.c_uint32), ("foldk_items", C.c_uint32), ("foldk_queries", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


FOLD_SELF_MAX_TERMS = 4                  # RHJ_FOLD_SELF_MAX_TERMS
QUERY_MAX_RELS = 8                       # RHJ_QUERY_MAX_RELS


class FoldEqTerm(C.Structure):
    """rhj_fold_eq_term (include/rhj_inter.h): colA[selA ? selA[i] : i] == colB[selB ? selB[i] : i]"""
    _fields_ = [("d_colA", C.c_void_p), ("d_selA", C.c_void_p), ("d_colB", C.c_void_p), ("d_selB", C.c_void_p)]


class FoldSelfOut(C.Structure):
    """rhj_fold_self_out (include/rhj_inter.h): one output of a batched fold item with no child"""
    _fields_ = [("p", FoldFactor), ("d_out", C.c_void_p), ("total", C.c_uint64)]


class FoldSelfDesc(C.Structure):
    """rhj_fold_self_desc (include/rhj_inter.h): one item of rhj_fold_self_batch_device"""
    _fields_ = [("n", C.c_uint64), ("nterms", C.c_int), ("nouts", C.c_int),
                ("terms", FoldEqTerm * FOLD_SELF_MAX_TERMS), ("outs", FoldSelfOut * FOLD_MAX_OUTS),
                ("rc", C.c_int), ("path", C.c_int)]


class FoldsPlan(C.Structure):
    """rhj_folds_plan (include/rhj_inter.h): what rhj_query_folds_plan returns of a query that folds"""
    _fields_ = [("root", C.c_int), ("nsteps", C.c_int), ("nself", C.c_int), ("steps", FoldKStep * (QUERY_MAX_RELS - 1)),
                ("self", C.c_int * (QUERY_MAX_RELS * FOLD_SELF_MAX_TERMS))]


class QueryBatchFoldSelfInfo(C.Structure):
    """rhj_query_batch_fold_self_info (include/rhj_inter.h): whether the last rhj_query_batch_device issued its
    rhj_fold_self_batch_device call, that call's items and the queries that folded only because of rhj_set_query_fold_self"""
    _fields_ = [("self_calls", C.c_uint32), ("self_items", C.c_uint32), ("self_queries", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class JoinFoldNDesc(C.Structure):
    """rhj_join_foldn_desc (include/rhj_inter.h): one item of rhj_join_foldn_batch_device"""
    _fields_ = [("nkeys", C.c_int),
                ("d_colR", C.c_void_p * FOLD_MAX_KEYS), ("d_selR", C.c_void_p * FOLD_MAX_KEYS), ("nR", C.c_uint64),
                ("d_colS", C.c_void_p * FOLD_MAX_KEYS), ("d_selS", C.c_void_p * FOLD_MAX_KEYS), ("nS", C.c_uint64),
                ("nvalues", C.c_int), ("nouts", C.c_int),
                ("values", FoldFactor * FOLD_MAX_VALUES), ("outs", FoldOut * FOLD_MAX_OUTS),
                ("rc", C.c_int), ("path", C.c_int)]


class FoldNPlan(C.Structure):
    """rhj_foldn_plan (include/rhj_inter.h): what rhj_query_foldn_plan returns"""
    _fields_ = [("levels", C.c_int), ("root", C.c_int), ("nsteps", C.c_int), ("nself", C.c_int), ("node", C.c_int * QUERY_MAX_RELS),
                ("steps", FoldKStep * (QUERY_MAX_RELS - 1)), ("self", C.c_int * (QUERY_MAX_RELS * FOLD_SELF_MAX_TERMS))]


class QueryBatchFoldNodesInfo(C.Structure):
    """rhj_query_batch_fold_nodes_info (include/rhj_inter.h): the rhj_join_foldn_batch_device calls the last
    rhj_query_batch_device issued and their items, the queries that handed over from levels to folds over nodes, and the levels
    they ran before"""
    _fields_ = [("foldn_calls", C.c_uint32), ("foldn_items", C.c_uint32), ("node_queries", C.c_uint32), ("node_levels", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


FILTER_MAX_TERMS = 4                     # RHJ_FILTER_MAX_TERMS


class FoldConstTerm(C.Structure):
    """rhj_fold_const_term (include/rhj_inter.h): col[sel ? sel[i] : i] op value, compared unsigned"""
    _fields_ = [("d_col", C.c_void_p), ("d_sel", C.c_void_p), ("op", C.c_char), ("value", C.c_uint64)]


class FoldPredDesc(C.Structure):
    """rhj_fold_pred_desc (include/rhj_inter.h): one item of rhj_fold_pred_batch_device"""
    _fields_ = [("n", C.c_uint64), ("nconst", C.c_int), ("neq", C.c_int), ("nouts", C.c_int),
                ("consts", FoldConstTerm * FILTER_MAX_TERMS), ("eqs", FoldEqTerm * FOLD_SELF_MAX_TERMS),
                ("outs", FoldSelfOut * FOLD_MAX_OUTS), ("rc", C.c_int), ("path", C.c_int)]


class QueryBatchOneWaitInfo(C.Structure):
    """rhj_query_batch_one_wait_info (include/rhj_inter.h): the queries the last rhj_query_batch_device ran as fold programs with
    one wait each, the programs, their items by kind, their rounds, launches, memsets and waits"""
    _fields_ = [(n, C.c_uint32) for n in ("queries", "programs", "pred_items", "fold_items", "foldk_items", "rounds", "launches", "memsets", "waits")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class QueryBatchProductsInfo(C.Structure):
    """rhj_query_batch_products_info (include/rhj_inter.h): the queries of several components (cross products) the last
    rhj_query_batch_device took, and their components"""
    _fields_ = [("product_queries", C.c_uint32), ("components", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class TableBatchCombineInfo(C.Structure):
    """rhj_table_batch_combine_info (include/rhj_inter.h): the add launches' tiles of the last table batch (or of the table
    batches inside the last rhj_query_batch_device) with rhj_set_fold_combine on, those that combined, and the device-scope adds
    into table slots they issued"""
    _fields_ = [("tiles", C.c_uint64), ("combined_tiles", C.c_uint64), ("slot_adds", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class TableBatchResidentInfo(C.Structure):
    """rhj_table_batch_resident_info (include/rhj_inter.h): the items of the last fold batch on one key (or of those inside the
    last rhj_query_batch_device) that one workgroup folded in LDS with rhj_set_fold_resident on, their launches, and the items
    that took the table form"""
    _fields_ = [("resident_items", C.c_uint32), ("resident_launches", C.c_uint32), ("table_items", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def query_components(lib, query, nrel=None):
    """rhj_query_components on one query (relations, joins, filters, views): [component of every binding], the components
    numbered 0, 1, ... in the order of their lowest binding (one component unless the query is a cross product); ValueError on -3"""
    arr, keep = query_descs([query])
    comp = (C.c_int * QUERY_MAX_RELS)()
    rc = lib.rhj_query_components(C.byref(arr[0]), nrel if nrel is not None else max(query[0]) + 1, None, comp)
    del keep
    if rc == -3:
        raise ValueError("rhj_query_components refused the query")
    got = list(comp[:len(query[0])])
    if rc != max(got) + 1:
        raise RuntimeError("rhj_query_components returned %d for the components %s" % (rc, got))
    return got


def query_one_wait_plan(lib, query, rels=None, nrel=None):
    """rhj_query_one_wait_plan on one query (relations, joins, filters, views): 1 when it takes the one-wait route under the
    switches and the row limit as they stand, 0 when it does not; ValueError on -3.  rels: a DeviceRelation array (the rule reads
    the relations' rows), or None."""
    arr, keep = query_descs([query])
    rc = lib.rhj_query_one_wait_plan(C.byref(arr[0]), nrel if nrel is not None else max(query[0]) + 1, rels)
    del keep
    if rc == -3:
        raise ValueError("rhj_query_one_wait_plan refused the query")
    return rc


def query_foldn_plan(lib, query, nrel=None):
    """rhj_query_foldn_plan on one query (relations, joins, filters, views): (levels, [node of every binding], root,
    [(child, parent, round, [predicate indices])], [indices of the kept predicates inside a node]); ValueError on -3"""
    arr, keep = query_descs([query])
    plan = FoldNPlan()
    rc = lib.rhj_query_foldn_plan(C.byref(arr[0]), nrel if nrel is not None else max(query[0]) + 1, None, C.byref(plan))
    del keep
    if rc == -3:
        raise ValueError("rhj_query_foldn_plan refused the query")
    if rc != 1:
        raise RuntimeError("rhj_query_foldn_plan found no hand-over (%d)" % rc)
    steps = [(s.child, s.parent, s.round, list(s.joins[:s.nkeys])) for s in plan.steps[:plan.nsteps]]
    return plan.levels, list(plan.node[:len(query[0])]), plan.root, steps, list(plan.self[:plan.nself])


def query_folds_plan(lib, query, nrel=None):
    """rhj_query_folds_plan on one query (relations, joins, filters, views): None when it does not fold, else
    (root, [(child, parent, round, [predicate indices])], [indices of the kept one-binding predicates]); ValueError on -3"""
    arr, keep = query_descs([query])
    plan = FoldsPlan()
    rc = lib.rhj_query_folds_plan(C.byref(arr[0]), nrel if nrel is not None else max(query[0]) + 1, None, C.byref(plan))
    del keep
    if rc == -3:
        raise ValueError("rhj_query_folds_plan refused the query")
    if rc != 1:
        return None
    steps = [(s.child, s.parent, s.round, list(s.joins[:s.nkeys])) for s in plan.steps[:plan.nsteps]]
    return plan.root, steps, list(plan.self[:plan.nself])


class QueryInfo(dict):
    """rhj_query_batch_last_info() as a dict, with rhj_query_batch_last_sum_info(), rhj_query_batch_last_fold_info(),
    rhj_query_batch_last_foldk_info() and rhj_query_batch_last_fold_self_info() as the dicts in its attributes sum_info,
    fold_info, foldk_info and fold_self_info, and rhj_query_batch_last_fold_nodes_info() in fold_nodes_info"""
    sum_info = None
    fold_info = None
    foldk_info = None
    fold_self_info = None
    fold_nodes_info = None
    one_wait_info = None
    products_info = None


def query_descs(queries):
    """(QueryDesc array, what keeps its pointers alive) of queries = [(relations, joins, filters, views), ...]: relations the
    relation index of every binding, joins [(a, ca, b, cb)], filters [(a, ca, op, value)], views [(a, c)], a and b bindings."""
    arr = (QueryDesc * max(len(queries), 1))()
    keep = []
    for d, (rels, joins, filters, views) in zip(arr, queries):
        r = (C.c_int * max(len(rels), 1))(*rels)
        f = (QueryFilter * max(len(filters), 1))(*[QueryFilter(a, c, op.encode(), int(v) & ((1 << 64) - 1)) for a, c, op, v in filters])
        j = (QueryJoin * max(len(joins), 1))(*[QueryJoin(*p) for p in joins])
        v = (QueryView * max(len(views), 1))(*[QueryView(*p) for p in views])
        keep.append((r, f, j, v))
        d.nrels, d.rels, d.nfilters, d.filters = len(rels), r, len(filters), f
        d.njoins, d.joins, d.nviews, d.views = len(joins), j, len(views), v
    return arr, keep


class Stats(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("ms_hist", "ms_scan", "ms_scatter", "ms_plan", "ms_build", "ms_count",
                                         "ms_offsets", "ms_probe", "ms_total", "ms_h2d", "ms_d2h")] + \
               [(n, C.c_uint64) for n in ("n_r", "n_s", "matches", "units", "hbm_units", "max_build", "table_slots")] + \
               [("radix_bits", C.c_int), ("reserved", C.c_int)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}
        r = self.reserved                  # path of the last join (include/rhj.h)
        d["path"] = {0: "tiled", 1: "fused", 3: "small", 4: "lowradix", 5: "subbucket", 6: "batch", 7: "filter_batch", 8: "apply_batch", 9: "eq2_batch", 10: "query_batch", 11: "stats_batch", 12: "join_sum_batch", 13: "join_fold_batch", 14: "join_foldk_batch", 15: "fold_self_batch", 16: "join_foldn_batch", 17: "fold_pred_batch"}.get(r & 0xff, "?")
        d["sub_bits"], d["pass1_bits"] = (r >> 8) & 0xff, (r >> 16) & 0xff
        return d


def build():
    """Compile librhj.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-s", "-C", HERE, "all"])


def load_library(path=None):
    LIB_PATH = path or os.environ.get("RHJ_LIB") or globals()["LIB_PATH"]      # RHJ_LIB: e.g. the diagnostics build, build/librhj_instr.so (`make instr`)
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("librhj.so is not built (run `make -C sigmod-2018_amd` or __graft_entry__.build()); "
                           "this package has no CPU fallback")
    # torch ships its own libamdhip64; load it first so that librhj.so binds to the HIP
    # runtime already in the process instead of pulling a second one from /opt/rocm
    # (two runtimes in one process: the second sees no device)
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    u64p = C.POINTER(C.c_uint64)
    L.RadixHashJoin.argtypes = [C.POINTER(Relation), C.POINTER(Relation), C.c_void_p]
    L.RadixHashJoin.restype = C.POINTER(Result)
    L.Filter.argtypes = [C.POINTER(InterRes), C.POINTER(FilterPred), C.POINTER(RelationMap), C.POINTER(C.c_int)]
    L.Filter.restype = C.POINTER(Result)
    L.FreeResult.argtypes = [C.POINTER(Result)]
    L.GetResultNum.argtypes = [C.POINTER(Result)]
    L.InsertResult.argtypes = [C.POINTER(C.POINTER(Result)), C.c_void_p]
    L.InsertResult.restype = C.POINTER(Result)
    L.InsertRowIdResult.argtypes = [C.POINTER(C.POINTER(Result)), u64p]
    L.InsertRowIdResult.restype = C.POINTER(Result)
    L.FindResultRowId.argtypes = [C.POINTER(Result), C.c_int]
    L.FindResultRowId.restype = C.c_uint64
    L.FindResultTuples.argtypes = [C.POINTER(Result), C.c_int]
    L.FindResultTuples.restype = C.c_void_p
    L.rhj_set_radix_bits.argtypes = [C.c_int]
    L.rhj_set_empty_mode.argtypes = [C.c_int]
    L.rhj_set_node_pairs.argtypes = [C.c_uint64]
    L.rhj_set_device.argtypes = [C.c_int]
    L.rhj_set_stream.argtypes = [C.c_void_p]
    L.rhj_set_force_hbm_table.argtypes = [C.c_int]
    L.rhj_set_fused.argtypes = [C.c_int]
    L.rhj_set_resident.argtypes = [C.c_int]
    L.rhj_set_small.argtypes = [C.c_int]
    L.rhj_set_lowradix.argtypes = [C.c_int]
    L.rhj_set_count_in_pass1.argtypes = [C.c_int]
    L.rhj_set_spec.argtypes = [C.c_int]
    L.rhj_last_spec.restype = C.c_int
    L.rhj_set_walk_count.argtypes = [C.c_int]
    L.rhj_last_walk_units.restype = C.c_int64
    if hasattr(L, "rhj_last_exact"):              # (A/B runs load earlier builds through this module too)
        L.rhj_last_exact.restype = C.c_int
    if hasattr(L, "rhj_set_devices"):
        L.rhj_set_devices.argtypes = [C.c_int]
        L.rhj_device_range.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.rhj_set_devices_balance.argtypes = [C.c_int]
        L.rhj_plan_device_ranges.argtypes = [u64p, u64p, C.c_int, C.c_int, C.POINTER(C.c_uint32)]
        if hasattr(L, "rhj_plan_device_slices"):
            L.rhj_plan_device_slices.argtypes = [u64p, u64p, C.c_int, C.c_int, C.POINTER(C.c_uint32), u64p]
            L.rhj_cut_to_slice.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), u64p, u64p]
            L.rhj_cut_to_slice.restype = None
            L.rhj_join_device_slice.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64,
                                                C.c_void_p, C.c_uint64, u64p]
        L.rhj_join_devices.argtypes = [C.POINTER(C.c_void_p), C.c_uint64, C.POINTER(C.c_void_p), C.c_uint64, C.POINTER(C.c_void_p), u64p, u64p]
        L.rhj_gather_pairs_devices.argtypes = [C.POINTER(C.c_void_p), u64p, C.c_int, C.c_void_p, C.c_uint64, u64p]
    L.rhj_set_order.argtypes = [C.c_int]
    L.rhj_get_order.restype = C.c_int
    L.rhj_auto_radix_bits.argtypes = [C.c_uint64, C.c_uint64]
    L.rhj_auto_radix_bits.restype = C.c_int
    L.rhj_sub_bits.argtypes = [C.c_int, C.c_uint64, C.c_uint64]
    L.rhj_sub_bits.restype = C.c_int
    L.rhj_set_timing.argtypes = [C.c_int]
    L.rhj_join_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p]
    if hasattr(L, "rhj_join_batch_device"):       # (A/B runs load earlier builds through this module too)
        L.rhj_join_batch_device.argtypes = [C.POINTER(JoinDesc), C.c_uint64]
        L.rhj_batch_takes.argtypes = [C.c_int, C.c_uint64, C.c_uint64]
        L.rhj_batch_takes.restype = C.c_int
    if hasattr(L, "rhj_join_cols_batch_device"):  # (A/B runs load earlier builds through this module too)
        L.rhj_join_cols_batch_device.argtypes = [C.POINTER(JoinColsDesc), C.c_uint64]
        L.rhj_join_cols_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p]
    L.rhj_build_relation_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    if hasattr(L, "rhj_join_keys_device"):
        L.rhj_join_keys_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p]
    L.rhj_partition_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rhj_filter_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char, C.c_uint64, C.c_void_p, u64p]
    if hasattr(L, "rhj_filter_batch_device"):     # (A/B runs load earlier builds through this module too)
        L.rhj_filter_batch_device.argtypes = [C.POINTER(FilterDesc), C.c_uint64]
        L.rhj_filter_batch_takes.argtypes = [C.c_uint64]
        L.rhj_filter_batch_takes.restype = C.c_int
    if hasattr(L, "rhj_apply_batch_device"):      # (A/B runs load earlier builds through this module too)
        L.rhj_apply_batch_device.argtypes = [C.POINTER(ApplyDesc), C.c_uint64]
    if hasattr(L, "rhj_query_batch_device"):      # (A/B runs load earlier builds through this module too)
        L.rhj_filter_eq2_batch_device.argtypes = [C.POINTER(Eq2Desc), C.c_uint64]
        L.rhj_query_batch_device.argtypes = [C.POINTER(DeviceRelation), C.c_int, C.POINTER(QueryDesc), C.c_uint64]
        L.rhj_query_levels.argtypes = [C.POINTER(QueryDesc), C.c_int, C.POINTER(DeviceRelation), C.POINTER(C.c_int)]
        L.rhj_query_batch_last_info.restype = C.POINTER(QueryBatchInfo)
    if hasattr(L, "rhj_column_stats_batch_device"):   # (A/B runs load earlier builds through this module too)
        L.rhj_column_stats_batch_device.argtypes = [C.POINTER(ColStatsDesc), C.c_uint64]
        L.rhj_column_stats_flags.argtypes = [C.c_uint64, C.c_uint64]
        L.rhj_column_stats_flags.restype = C.c_uint64
        L.rhj_column_stats_batch_last_info.restype = C.POINTER(ColStatsBatchInfo)
    if hasattr(L, "rhj_join_sum_batch_device"):       # (A/B runs load earlier builds through this module too)
        L.rhj_join_sum_batch_device.argtypes = [C.POINTER(JoinSumDesc), C.c_uint64]
        L.rhj_set_query_sum_last.argtypes = [C.c_int]
        L.rhj_set_query_sum_last.restype = None
        L.rhj_query_batch_last_sum_info.restype = C.POINTER(QueryBatchSumInfo)
    if hasattr(L, "rhj_join_fold_batch_device"):
        L.rhj_join_fold_batch_device.argtypes = [C.POINTER(JoinFoldDesc), C.c_uint64]
        L.rhj_query_fold_plan.argtypes = [C.POINTER(QueryDesc), C.c_int, C.POINTER(DeviceRelation), C.POINTER(C.c_int), C.POINTER(FoldStep)]
        L.rhj_set_query_fold.argtypes = [C.c_int]
        L.rhj_set_query_fold.restype = None
        L.rhj_query_batch_last_fold_info.restype = C.POINTER(QueryBatchFoldInfo)
    if hasattr(L, "rhj_join_foldk_batch_device"):     # (A/B runs load earlier builds through this module too)
        L.rhj_join_foldk_batch_device.argtypes = [C.POINTER(JoinFoldKDesc), C.c_uint64]
        L.rhj_query_foldk_plan.argtypes = [C.POINTER(QueryDesc), C.c_int, C.POINTER(DeviceRelation), C.POINTER(C.c_int), C.POINTER(FoldKStep)]
        L.rhj_set_query_fold_keys.argtypes = [C.c_int]
        L.rhj_set_query_fold_keys.restype = None
        L.rhj_query_batch_last_foldk_info.restype = C.POINTER(QueryBatchFoldKInfo)
    if hasattr(L, "rhj_fold_self_batch_device"):
        L.rhj_fold_self_batch_device.argtypes = [C.POINTER(FoldSelfDesc), C.c_uint64]
        L.rhj_query_folds_plan.argtypes = [C.POINTER(QueryDesc), C.c_int, C.POINTER(DeviceRelation), C.POINTER(FoldsPlan)]
        L.rhj_set_query_fold_self.argtypes = [C.c_int]
        L.rhj_set_query_fold_self.restype = None
        L.rhj_query_batch_last_fold_self_info.restype = C.POINTER(QueryBatchFoldSelfInfo)
    if hasattr(L, "rhj_join_foldn_batch_device"):     # (A/B runs load earlier builds through this module too)
        L.rhj_join_foldn_batch_device.argtypes = [C.POINTER(JoinFoldNDesc), C.c_uint64]
        L.rhj_query_foldn_plan.argtypes = [C.POINTER(QueryDesc), C.c_int, C.POINTER(DeviceRelation), C.POINTER(FoldNPlan)]
        L.rhj_set_query_fold_nodes.argtypes = [C.c_int]
        L.rhj_set_query_fold_nodes.restype = None
        L.rhj_set_query_fold_node_rows.argtypes = [C.c_uint64]
        L.rhj_set_query_fold_node_rows.restype = None
        L.rhj_query_batch_last_fold_nodes_info.restype = C.POINTER(QueryBatchFoldNodesInfo)
    if hasattr(L, "rhj_fold_pred_batch_device"):      # (A/B runs load earlier builds through this module too)
        L.rhj_fold_pred_batch_device.argtypes = [C.POINTER(FoldPredDesc), C.c_uint64]
        L.rhj_query_one_wait_plan.argtypes = [C.POINTER(QueryDesc), C.c_int, C.POINTER(DeviceRelation)]
        L.rhj_set_query_fold_one_wait.argtypes = [C.c_int]
        L.rhj_set_query_fold_one_wait.restype = None
        L.rhj_set_query_fold_one_wait_rows.argtypes = [C.c_uint64]
        L.rhj_set_query_fold_one_wait_rows.restype = None
        L.rhj_query_batch_last_one_wait_info.restype = C.POINTER(QueryBatchOneWaitInfo)
    if hasattr(L, "rhj_query_components"):            # (A/B runs load earlier builds through this module too)
        L.rhj_query_components.argtypes = [C.POINTER(QueryDesc), C.c_int, C.POINTER(DeviceRelation), C.POINTER(C.c_int)]
        L.rhj_set_query_products.argtypes = [C.c_int]
        L.rhj_set_query_products.restype = None
        L.rhj_query_batch_last_products_info.restype = C.POINTER(QueryBatchProductsInfo)
    if hasattr(L, "rhj_set_fold_combine"):            # (A/B runs load earlier builds through this module too)
        L.rhj_set_fold_combine.argtypes = [C.c_int]
        L.rhj_set_fold_combine.restype = None
        L.rhj_get_fold_combine.restype = C.c_int
        L.rhj_table_batch_last_combine_info.restype = C.POINTER(TableBatchCombineInfo)
    if hasattr(L, "rhj_set_fold_resident"):           # (A/B runs load earlier builds through this module too)
        L.rhj_set_fold_resident.argtypes = [C.c_int]
        L.rhj_set_fold_resident.restype = None
        L.rhj_get_fold_resident.restype = C.c_int
        L.rhj_fold_resident_rule.argtypes = [C.c_uint64, C.c_uint64, C.c_int]
        L.rhj_fold_resident_rule.restype = C.c_int
        L.rhj_table_batch_last_resident_info.restype = C.POINTER(TableBatchResidentInfo)
    if hasattr(L, "rhj_set_fold_resident_keys"):
        L.rhj_set_fold_resident_keys.argtypes = [C.c_int]
        L.rhj_set_fold_resident_keys.restype = None
        L.rhj_get_fold_resident_keys.restype = C.c_int
        L.rhj_fold_resident_keys_rule.argtypes = [C.c_uint64, C.c_uint64, C.c_int]
        L.rhj_fold_resident_keys_rule.restype = C.c_int
        L.rhj_table_batch_last_resident_keys_info.restype = C.POINTER(TableBatchResidentInfo)
    L.rhj_register_relation_map.argtypes = [C.POINTER(RelationMap), C.c_int]
    L.rhj_unregister_relation_map.argtypes = [C.POINTER(RelationMap), C.c_int]
    L.rhj_bucket_histogram_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    L.rhj_select_bucket_range_device.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, u64p]
    L.rhj_join_device_range.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, u64p]
    L.rhj_pin_refusals.restype = C.c_int
    L.rhj_last_stats.restype = C.POINTER(Stats)
    L.rhj_version.restype = C.c_char_p
    return L


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class RHJ:
    """Device and host entry points of librhj.so."""

    def __init__(self, device=None, use_torch_stream=True, lib_path=None):
        import torch
        self.torch = torch
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the radix hash join has no CPU path")
        self.lib = load_library(lib_path)
        if device is not None:
            if self.lib.rhj_set_device(int(device)) != 0 and self.lib.rhj_get_device() != int(device):
                raise RuntimeError("librhj.so already runs on device %d: one library context per process "
                                   "(rhj_set_device(%d) refused)" % (self.lib.rhj_get_device(), int(device)))
            torch.cuda.set_device(int(device))
        self.dev = torch.device("cuda", torch.cuda.current_device())
        if use_torch_stream:
            self.lib.rhj_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))

    # ---- knobs
    def set_bits(self, bits):
        if self.lib.rhj_set_radix_bits(int(bits)) != 0:
            raise ValueError("radix bits out of range: %r" % (bits,))

    def stats(self):
        return self.lib.rhj_last_stats().contents.as_dict()

    # ---- device-resident API
    def to_device(self, rel):
        """numpy TUPLE array -> int64 tensor [n,2] on the device (same bytes)."""
        rel = np.ascontiguousarray(rel, dtype=TUPLE)
        t = self.torch.from_numpy(rel.view(np.int64).reshape(-1, 2).copy())
        return t.to(self.dev)

    def join_device(self, dR, dS, capacity=None, count_only=False, bucket_range=None):
        """dR, dS: int64 tensors [n,2] (value,row_id).  Returns (pairs tensor [M,2], matches).
        bucket_range = (lo, hi): only the buckets [lo, hi) of the current radix (rhj_join_device_range: one rank's share of a
        sharded join; the partition drops the other buckets while it reads the relations); (lo, hi, first_skip, last_end): a share
        cut inside its first / last bucket (rhj_join_device_slice)."""
        torch = self.torch
        nR, nS = dR.shape[0], dS.shape[0]
        m = C.c_uint64(0)

        def call(out_ptr, cap):
            if bucket_range is None:
                rc = self.lib.rhj_join_device(dR.data_ptr(), nR, dS.data_ptr(), nS, out_ptr, cap, C.byref(m))
            elif len(bucket_range) == 4:
                rc = self.lib.rhj_join_device_slice(dR.data_ptr(), nR, dS.data_ptr(), nS, int(bucket_range[0]), int(bucket_range[1]),
                                                    int(bucket_range[2]), int(bucket_range[3]), out_ptr, cap, C.byref(m))
            else:
                rc = self.lib.rhj_join_device_range(dR.data_ptr(), nR, dS.data_ptr(), nS, int(bucket_range[0]), int(bucket_range[1]),
                                                    out_ptr, cap, C.byref(m))
            if rc < 0:
                raise RuntimeError("rhj_join_device failed (%d)" % rc)

        if count_only:
            call(None, 0)
            return None, m.value
        if capacity is None:
            call(None, 0)
            capacity = m.value
        out = torch.empty((max(capacity, 1), 2), dtype=torch.int64, device=self.dev)
        call(out.data_ptr(), capacity)
        return out[:min(m.value, capacity)], m.value

    def join_batch_device(self, pairs_of_tensors, capacities=None, count_only=False, with_info=False):
        """Many independent joins in one call (rhj_join_batch_device): pairs_of_tensors = [(dR, dS), ...], int64 tensors [n,2]
        as for join_device; inputs may be shared between joins.  Returns [(pairs tensor [M,2], matches), ...] with join_device's
        conventions: count_only gives (None, matches); capacities[i] given: at most that many pairs of join i are written and
        returned; capacities None: every join gets room for max(nR, nS) pairs, and the joins that needed more run again, with
        room for their count, in a second batched call.  with_info: also the list of the joins' path ids (6: batched)."""
        torch = self.torch
        n = len(pairs_of_tensors)
        descs = (JoinDesc * max(n, 1))()
        outs = [None] * n

        def call(which, caps):
            arr = (JoinDesc * max(len(which), 1))()
            for k, i in enumerate(which):
                dR, dS = pairs_of_tensors[i]
                d = arr[k]
                d.d_R, d.nR, d.d_S, d.nS = dR.data_ptr(), dR.shape[0], dS.data_ptr(), dS.shape[0]
                if caps is not None:
                    outs[i] = torch.empty((max(int(caps[k]), 1), 2), dtype=torch.int64, device=self.dev)
                    d.d_out, d.out_capacity = outs[i].data_ptr(), int(caps[k])
            rc = self.lib.rhj_join_batch_device(arr, len(which))
            if rc < 0:
                raise RuntimeError("rhj_join_batch_device failed (%d)" % rc)
            for k, i in enumerate(which):
                descs[i] = arr[k]
            return rc

        everything = list(range(n))
        if count_only:
            call(everything, None)
        elif capacities is not None:
            call(everything, [int(c) for c in capacities])
        else:
            call(everything, [max(dR.shape[0], dS.shape[0]) for dR, dS in pairs_of_tensors])
            short = [i for i in everything if descs[i].rc == 1]
            if short:                               # fan-out above the guess: the counts are known now
                call(short, [descs[i].matches for i in short])
        res = []
        for i in everything:
            d = descs[i]
            res.append((None, d.matches) if count_only else (outs[i][:min(d.matches, d.out_capacity)], d.matches))
        return (res, [descs[i].path for i in everything]) if with_info else res

    @staticmethod
    def _cols_side(col, sel):
        """(column pointer, vector pointer or None, tuples) of one side of a join on columns"""
        return col.data_ptr(), (sel.data_ptr() if sel is not None else None), (col.shape[0] if sel is None else sel.shape[0])

    def join_cols_batch_device(self, joins, capacities=None, count_only=False, with_info=False):
        """Many independent joins on key columns read through row-id vectors (rhj_join_cols_batch_device): joins =
        [(colR, selR, colS, selS), ...], int64 tensors [n]; a vector may be None (the whole column), and tuple i of a side is
        (col[sel[i]], i).  Columns and vectors may be shared.  Returns what join_batch_device returns, by the same protocol:
        count_only gives (None, matches); capacities[i] given: at most that many pairs of join i are written and returned;
        capacities None: every join gets room for max(nR, nS) pairs, and the joins that needed more run again, with room for
        their count, in a second batched call.  with_info: also the list of the joins' path ids (6: batched)."""
        torch = self.torch
        n = len(joins)
        descs = (JoinColsDesc * max(n, 1))()
        outs = [None] * n
        sizes = [(self._cols_side(cR, sR)[2], self._cols_side(cS, sS)[2]) for cR, sR, cS, sS in joins]

        def call(which, caps):
            arr = (JoinColsDesc * max(len(which), 1))()
            for k, i in enumerate(which):
                cR, sR, cS, sS = joins[i]
                d = arr[k]
                d.d_colR, d.d_selR, d.nR = self._cols_side(cR, sR)
                d.d_colS, d.d_selS, d.nS = self._cols_side(cS, sS)
                if caps is not None:
                    outs[i] = torch.empty((max(int(caps[k]), 1), 2), dtype=torch.int64, device=self.dev)
                    d.d_out, d.out_capacity = outs[i].data_ptr(), int(caps[k])
            rc = self.lib.rhj_join_cols_batch_device(arr, len(which))
            if rc < 0:
                raise RuntimeError("rhj_join_cols_batch_device failed (%d)" % rc)
            for k, i in enumerate(which):
                descs[i] = arr[k]
            return rc

        everything = list(range(n))
        if count_only:
            call(everything, None)
        elif capacities is not None:
            call(everything, [int(c) for c in capacities])
        else:
            call(everything, [max(nR, nS) for nR, nS in sizes])
            short = [i for i in everything if descs[i].rc == 1]
            if short:                               # fan-out above the guess: the counts are known now
                call(short, [descs[i].matches for i in short])
        res = []
        for i in everything:
            d = descs[i]
            res.append((None, d.matches) if count_only else (outs[i][:min(d.matches, d.out_capacity)], d.matches))
        return (res, [descs[i].path for i in everything]) if with_info else res

    def join_cols_device(self, colR, selR, colS, selS, capacity=None, count_only=False):
        """One join on key columns read through row-id vectors (rhj_join_cols_device); arguments as one entry of
        join_cols_batch_device, result and capacity conventions as join_device."""
        torch = self.torch
        pR, vR, nR = self._cols_side(colR, selR)
        pS, vS, nS = self._cols_side(colS, selS)
        m = C.c_uint64(0)

        def call(out_ptr, cap):
            rc = self.lib.rhj_join_cols_device(pR, vR, nR, pS, vS, nS, out_ptr, cap, C.byref(m))
            if rc < 0:
                raise RuntimeError("rhj_join_cols_device failed (%d)" % rc)

        if count_only:
            call(None, 0)
            return None, m.value
        if capacity is None:
            call(None, 0)
            capacity = m.value
        out = torch.empty((max(capacity, 1), 2), dtype=torch.int64, device=self.dev)
        call(out.data_ptr(), capacity)
        return out[:min(m.value, capacity)], m.value

    def partition_device(self, d_in, bits=None):
        torch = self.torch
        if bits is not None:
            self.set_bits(bits)
        bits = self.lib.rhj_get_radix_bits()
        out = torch.empty_like(d_in)
        hist = np.zeros(1 << bits, dtype=np.uint64)
        psum = np.zeros(1 << bits, dtype=np.int64)
        rc = self.lib.rhj_partition_device(d_in.data_ptr(), d_in.shape[0], out.data_ptr(), _np_ptr(hist), _np_ptr(psum))
        if rc < 0:
            raise RuntimeError("rhj_partition_device failed (%d)" % rc)
        return out, hist, psum

    def filter_device(self, d_col, op, value, d_sel=None):
        torch = self.torch
        n = d_col.shape[0] if d_sel is None else d_sel.shape[0]
        out = torch.empty(max(n, 1), dtype=torch.int64, device=self.dev)
        hits = C.c_uint64(0)
        k = int(value) & ((1 << 64) - 1)
        rc = self.lib.rhj_filter_device(d_col.data_ptr(), d_sel.data_ptr() if d_sel is not None else None, n,
                                        op.encode(), k, out.data_ptr(), C.byref(hits))
        if rc < 0:
            raise RuntimeError("rhj_filter_device failed (%d)" % rc)
        return out[:hits.value]

    def _mask_batch(self, entry, arr, n, count_only, with_info):
        """The second half of filter_batch_device and filter_eq2_batch_device: arr[0..n) has every field but d_out.  Places the
        items' outputs in one allocation, calls the entry point and returns the result list (and the path ids)."""
        out = None
        if not count_only:
            starts = np.concatenate([[0], np.cumsum([(arr[i].n + 1) // 2 * 2 for i in range(n)])]).astype(np.int64)      # 16-byte aligned pieces
            out = self.torch.empty(max(int(starts[-1]), 1), dtype=self.torch.int64, device=self.dev)
            for i in range(n):
                arr[i].d_out = out.data_ptr() + 8 * int(starts[i])
        rc = getattr(self.lib, entry)(arr, n)
        if rc < 0:
            raise RuntimeError("%s failed (%d)" % (entry, rc))
        res = [(None, arr[i].hits) if count_only else (out[int(starts[i]):int(starts[i]) + arr[i].hits], arr[i].hits) for i in range(n)]
        return (res, [arr[i].path for i in range(n)]) if with_info else res

    def filter_batch_device(self, filters, count_only=False, with_info=False):
        """Many independent conjunctive filters in one call (rhj_filter_batch_device): filters = [(terms, d_sel), ...] with
        terms = [(d_col, op, value), ...] (1..4 of them, columns of one relation; int64 tensors as for filter_device) and
        d_sel a row-id vector or None.  Returns [(indices tensor, hits), ...], or (None, hits) with count_only; the index lists
        are views of one allocation.  with_info: also the list of the filters' path ids (7: batched)."""
        n = len(filters)
        arr = (FilterDesc * max(n, 1))()
        for d, (terms, d_sel) in zip(arr, filters):
            if not 1 <= len(terms) <= FILTER_MAX_TERMS:
                raise ValueError("a filter has 1..%d terms, not %d" % (FILTER_MAX_TERMS, len(terms)))
            d.d_sel = d_sel.data_ptr() if d_sel is not None else None
            d.n = terms[0][0].shape[0] if d_sel is None else d_sel.shape[0]
            d.nterms = len(terms)
            for t, (d_col, op, value) in zip(d.terms, terms):
                t.d_col, t.op, t.value = d_col.data_ptr(), op.encode(), int(value) & ((1 << 64) - 1)
        return self._mask_batch("rhj_filter_batch_device", arr, n, count_only, with_info)

    def apply_batch_device(self, items, with_info=False):
        """Many row-id rebuilds and view sums in one call (rhj_apply_batch_device, include/rhj_inter.h): items =
        [(idx or None, stride, n, terms), ...] with idx an int64 tensor that holds an index list ([n] with stride 1, a pair list
        [n, 2] or a view of one with stride 2) and terms = [(side, src or None, want_rows, col or None), ...] (1..8 of them).
        Row i of a term is q = src[p] (p itself without src), p = idx[i * stride + side] (i itself without idx).  Returns per
        item a list of (rows tensor or None, sum or None): the n gathered ids where want_rows, the wrap-around sum of col[q]
        as a Python int below 2^64 where col is given.  The row tensors are views of one allocation.  with_info: also the
        list of the items' path ids (8: the batched launch, 0: an empty item)."""
        torch = self.torch
        n = len(items)
        arr = (ApplyDesc * max(n, 1))()
        places, lists, at = [], [], 0
        for d, (idx, stride, rows, terms) in zip(arr, items):
            if not 1 <= len(terms) <= APPLY_MAX_TERMS:
                raise ValueError("an item has 1..%d terms, not %d" % (APPLY_MAX_TERMS, len(terms)))
            d.d_idx = idx.data_ptr() if idx is not None else None
            d.n, d.idx_stride, d.nterms = int(rows), int(stride), len(terms)
            if idx is not None and idx.numel() == 0 and int(rows):
                raise ValueError("an empty index list for %d rows" % int(rows))
            lists.append(idx is not None)
            mine = []
            for t, (side, src, want_rows, col) in zip(d.terms, terms):
                t.side = int(side)
                t.d_src = src.data_ptr() if src is not None else None
                t.d_col = col.data_ptr() if col is not None else None
                mine.append(at if want_rows else None)
                if want_rows:
                    at += (int(rows) + 1) // 2 * 2               # 16-byte aligned pieces
            places.append(mine)
        out = torch.empty(max(at, 1), dtype=torch.int64, device=self.dev)
        for d, mine, listed in zip(arr, places, lists):
            for t, a in zip(d.terms, mine):
                if a is not None:
                    t.d_dst = out.data_ptr() + 8 * a
            if listed and not d.d_idx:                           # an empty tensor has no address: the list of a join without a
                d.d_idx = out.data_ptr()                         # match is still a list (side 1 is legal), and none of it is read
        rc = self.lib.rhj_apply_batch_device(arr, n)
        if rc < 0:
            raise RuntimeError("rhj_apply_batch_device failed (%d)" % rc)
        res = []
        for i in range(n):
            d = arr[i]
            res.append([(out[a:a + d.n] if a is not None else None, d.terms[k].sum if d.terms[k].d_col else None)
                        for k, a in enumerate(places[i])])
        return (res, [arr[i].path for i in range(n)]) if with_info else res

    def join_sum_batch_device(self, items, with_info=False):
        """The row counts and view sums of many final joins in one call, without their pairs (rhj_join_sum_batch_device,
        include/rhj_inter.h): items = [(colR, selR, colS, selS, terms), ...] as join_cols_batch_device takes the four, with
        terms = [(side, src or None, col), ...] (0..8 of them; side 0: R's position, 1: S's).  Returns [(matches, sums), ...]:
        the number of pairs and the wrap-around sums of col[src[p]] over them as Python ints below 2^64.  with_info: also the
        list of the items' path ids (12: the batched launches, 0: an item with an empty side)."""
        n = len(items)
        arr = (JoinSumDesc * max(n, 1))()
        for d, (cR, sR, cS, sS, terms) in zip(arr, items):
            if len(terms) > JOIN_SUM_MAX_TERMS:
                raise ValueError("an item has 0..%d terms, not %d" % (JOIN_SUM_MAX_TERMS, len(terms)))
            d.d_colR, d.d_selR, d.nR = self._cols_side(cR, sR)
            d.d_colS, d.d_selS, d.nS = self._cols_side(cS, sS)
            d.nterms = len(terms)
            for t, (side, src, col) in zip(d.terms, terms):
                t.side, t.d_src, t.d_col = int(side), (src.data_ptr() if src is not None else None), col.data_ptr()
        rc = self.lib.rhj_join_sum_batch_device(arr, n)
        if rc < 0:
            raise RuntimeError("rhj_join_sum_batch_device failed (%d)" % rc)
        res = [(arr[i].matches, [arr[i].terms[t].sum for t in range(arr[i].nterms)]) for i in range(n)]
        return (res, [arr[i].path for i in range(n)]) if with_info else res

    def set_query_sum_last(self, on):
        """query_batch_device takes every query's last join as its row count and view sums, without its pairs (default off)"""
        self.lib.rhj_set_query_sum_last(1 if on else 0)

    def join_foldk_batch_device(self, items, with_info=False):
        """join_fold_batch_device on tuple keys (rhj_join_foldk_batch_device, include/rhj_inter.h): items as there, but colR and
        colS are lists of 1..4 key columns, word t of R against word t of S, all of a side read through its one row-id vector.
        Path id 14 (19: one workgroup with the table in LDS, set_fold_resident_keys)."""
        return self._fold_batch(JoinFoldKDesc, "rhj_join_foldk_batch_device", items, with_info)

    def join_foldn_batch_device(self, items, with_info=False):
        """join_foldk_batch_device with a row-id vector per key word (rhj_join_foldn_batch_device, include/rhj_inter.h): items as
        there, but selR and selS are lists with one vector or None per key column; word t of a side's position p is
        col[t][sel[t][p]] (col[t][p] without a vector).  A side's positions are the length of its first vector, or of its first
        column when it has none.  Path id 16 (19: one workgroup with the table in LDS, set_fold_resident_keys)."""
        return self._fold_batch(JoinFoldNDesc, "rhj_join_foldn_batch_device", items, with_info)

    def set_query_fold_nodes(self, on):
        """with set_query_fold, set_query_fold_keys and set_query_fold_self all on: a query none of them takes runs as levels only
        until its merged nodes and remaining predicates form a tree, and folds over the nodes from there (default off)"""
        self.lib.rhj_set_query_fold_nodes(1 if on else 0)

    def set_query_fold_node_rows(self, limit):
        """a query hands over to the folds over nodes only while its merged nodes have fewer rows than this (default and most 2^32)"""
        self.lib.rhj_set_query_fold_node_rows(int(limit))

    def set_query_fold_keys(self, on):
        """with set_query_fold: the queries whose predicates are a tree once several predicates between two bindings are read as
        one join on a tuple of columns fold too (default off)"""
        self.lib.rhj_set_query_fold_keys(1 if on else 0)

    def fold_self_batch_device(self, items, with_info=False):
        """Many folds with no child in one call (rhj_fold_self_batch_device, include/rhj_inter.h): items =
        [(n, terms, outs), ...] with terms = [(colA, selA, colB, selB), ...] (0..4 equalities, int64 tensors, a vector may be
        None) and outs = [((w, src, col), out), ...] (0..9 of them: a factor over the side's positions, and out = None for the
        total only, True for a vector of this call's, or an int64 tensor of at least n elements to write into).  Returns per
        item a list of (vector or None, total): d_out[i] = m(i) * P(i) and its sum, Python ints below 2^64.  The vectors this
        call makes are views of one allocation.  with_info: also the list of the items' path ids (15: the batched launch, 0:
        an item without rows, whose vectors are left as they were)."""
        torch = self.torch
        ptr = lambda t: t.data_ptr() if t is not None else None
        n = len(items)
        arr = (FoldSelfDesc * max(n, 1))()
        places, at = [], 0
        for d, (rows, terms, outs) in zip(arr, items):
            if len(terms) > FOLD_SELF_MAX_TERMS or len(outs) > FOLD_MAX_OUTS:
                raise ValueError("an item has 0..%d terms and 0..%d outputs, not %d and %d" % (FOLD_SELF_MAX_TERMS, FOLD_MAX_OUTS, len(terms), len(outs)))
            d.n, d.nterms, d.nouts = int(rows), len(terms), len(outs)
            for t, (colA, selA, colB, selB) in zip(d.terms, terms):
                t.d_colA, t.d_selA, t.d_colB, t.d_selB = ptr(colA), ptr(selA), ptr(colB), ptr(selB)
            mine = []
            for o, ((w, src, col), out) in zip(d.outs, outs):
                o.p.d_w, o.p.d_src, o.p.d_col = ptr(w), ptr(src), ptr(col)
                if out is True:
                    mine.append(at)
                    at += (d.n + 1) // 2 * 2                     # 16-byte aligned pieces
                else:
                    if out is not None and out.numel() < d.n:
                        raise ValueError("an output vector of %d words for %d rows" % (out.numel(), d.n))
                    mine.append(out)
            places.append(mine)
        buf = torch.zeros(max(at, 1), dtype=torch.int64, device=self.dev)
        for d, mine in zip(arr, places):
            for o, a in zip(d.outs, mine):
                o.d_out = None if a is None else buf.data_ptr() + 8 * a if isinstance(a, int) else a.data_ptr()
        rc = self.lib.rhj_fold_self_batch_device(arr, n)
        if rc < 0:
            raise RuntimeError("rhj_fold_self_batch_device failed (%d)" % rc)
        res = []
        for d, mine in zip(arr, places):
            res.append([(None if a is None else buf[a:a + d.n] if isinstance(a, int) else a[:d.n], d.outs[k].total) for k, a in enumerate(mine)])
        return (res, [arr[i].path for i in range(n)]) if with_info else res

    def fold_pred_batch_device(self, items, with_info=False):
        """fold_self_batch_device with constant predicates (rhj_fold_pred_batch_device, include/rhj_inter.h): items =
        [(n, consts, eqs, outs), ...] with consts = [(col, sel, op, value), ...] (0..4 comparisons col[sel[i]] op value, op one of
        "<", ">", "=", compared unsigned, sel a vector or None), eqs and outs as fold_self_batch_device's terms and outs.  Returns
        per item a list of (vector or None, total).  with_info: also the list of the items' path ids (17: the batched launch, 0:
        an item without rows, whose vectors are left as they were)."""
        torch = self.torch
        ptr = lambda t: t.data_ptr() if t is not None else None
        n = len(items)
        arr = (FoldPredDesc * max(n, 1))()
        places, at = [], 0
        for d, (rows, consts, eqs, outs) in zip(arr, items):
            if len(consts) > FILTER_MAX_TERMS or len(eqs) > FOLD_SELF_MAX_TERMS or len(outs) > FOLD_MAX_OUTS:
                raise ValueError("an item has 0..%d constant terms, 0..%d equalities and 0..%d outputs, not %d, %d and %d"
                                 % (FILTER_MAX_TERMS, FOLD_SELF_MAX_TERMS, FOLD_MAX_OUTS, len(consts), len(eqs), len(outs)))
            d.n, d.nconst, d.neq, d.nouts = int(rows), len(consts), len(eqs), len(outs)
            for t, (col, sel, op, value) in zip(d.consts, consts):
                t.d_col, t.d_sel, t.op, t.value = ptr(col), ptr(sel), op.encode(), int(value) & ((1 << 64) - 1)
            for t, (colA, selA, colB, selB) in zip(d.eqs, eqs):
                t.d_colA, t.d_selA, t.d_colB, t.d_selB = ptr(colA), ptr(selA), ptr(colB), ptr(selB)
            mine = []
            for o, ((w, src, col), out) in zip(d.outs, outs):
                o.p.d_w, o.p.d_src, o.p.d_col = ptr(w), ptr(src), ptr(col)
                if out is True:
                    mine.append(at)
                    at += (d.n + 1) // 2 * 2                     # 16-byte aligned pieces
                else:
                    if out is not None and out.numel() < d.n:
                        raise ValueError("an output vector of %d words for %d rows" % (out.numel(), d.n))
                    mine.append(out)
            places.append(mine)
        buf = torch.zeros(max(at, 1), dtype=torch.int64, device=self.dev)
        for d, mine in zip(arr, places):
            for o, a in zip(d.outs, mine):
                o.d_out = None if a is None else buf.data_ptr() + 8 * a if isinstance(a, int) else a.data_ptr()
        rc = self.lib.rhj_fold_pred_batch_device(arr, n)
        if rc < 0:
            raise RuntimeError("rhj_fold_pred_batch_device failed (%d)" % rc)
        res = []
        for d, mine in zip(arr, places):
            res.append([(None if a is None else buf[a:a + d.n] if isinstance(a, int) else a[:d.n], d.outs[k].total) for k, a in enumerate(mine)])
        return (res, [arr[i].path for i in range(n)]) if with_info else res

    def set_query_fold_one_wait(self, on):
        """with set_query_fold: the folding queries whose relations all have 1..set_query_fold_one_wait_rows' limit of rows run
        as fold programs: filters as 0/1 weights over whole relations, every round's launches queued behind one upload, and one
        wait a program (default off)"""
        self.lib.rhj_set_query_fold_one_wait(1 if on else 0)

    def set_query_fold_one_wait_rows(self, limit):
        """a query takes the one-wait route only while every binding's relation has at most this many rows (default 4096)"""
        self.lib.rhj_set_query_fold_one_wait_rows(int(limit))

    def set_query_products(self, on):
        """query_batch_device takes a query whose bindings end in several components, a cross product, as one query per
        component in the same batch and multiplies their rows and sums on the host; nothing of the product is built (default
        off: such a query is refused)"""
        self.lib.rhj_set_query_products(1 if on else 0)

    def set_query_fold_self(self, on):
        """with set_query_fold: the queries that fold once their one-binding predicates are 0/1 factors on a binding's weight and
        their implied predicates are dropped fold too, queries without a join among them (default off)"""
        self.lib.rhj_set_query_fold_self(1 if on else 0)

    def join_fold_batch_device(self, items, with_info=False):
        """Many weighted join folds in one call (rhj_join_fold_batch_device, include/rhj_inter.h): items =
        [(colR, selR, colS, selS, values, outs), ...] as join_cols_batch_device takes the four (R the parent side, S the
        child), values = [(w, src, col), ...] (0..9 factors over S's positions, each of the three an int64 tensor or None) and
        outs = [(value, (w, src, col), out), ...] (0..9 of them: a value index, a factor over R's positions, and out = None
        for the total only, True for a vector of this call's, or an int64 tensor of at least nR elements to write into).
        Returns per item a list of (vector or None, total): d_out[i] = P(i) * A_value(keyR(i)) and its sum, Python ints below
        2^64.  The vectors this call makes are views of one allocation.  with_info: also the list of the items' path ids (13:
        the batched launches, 18: one workgroup with the table in LDS, set_fold_resident, 0: an item with an empty side, whose vectors are left as they were)."""
        return self._fold_batch(JoinFoldDesc, "rhj_join_fold_batch_device", items, with_info)

    def _fold_batch(self, Desc, entry, items, with_info):
        """the fold batches: their items differ in the key columns and row-id vectors alone"""
        torch = self.torch
        ptr = lambda t: t.data_ptr() if t is not None else None
        n = len(items)
        arr = (Desc * max(n, 1))()
        places, at = [], 0
        for d, (cR, sR, cS, sS, values, outs) in zip(arr, items):
            if len(values) > FOLD_MAX_VALUES or len(outs) > FOLD_MAX_OUTS:
                raise ValueError("an item has 0..%d values and 0..%d outputs, not %d and %d" % (FOLD_MAX_VALUES, FOLD_MAX_OUTS, len(values), len(outs)))
            if Desc is JoinFoldNDesc:
                if not 1 <= len(cR) <= FOLD_MAX_KEYS or not len(cS) == len(cR) == len(sR) == len(sS):
                    raise ValueError("an item has 1..%d key columns a side, as many on both, each with a vector or None, not %d and %d" % (FOLD_MAX_KEYS, len(cR), len(cS)))
                d.nkeys = len(cR)
                for cols, sels, d_col, d_sel, side in ((cR, sR, d.d_colR, d.d_selR, "nR"), (cS, sS, d.d_colS, d.d_selS, "nS")):
                    given = [s for s in sels if s is not None]
                    rows = given[0].shape[0] if given else cols[0].shape[0]
                    if any(s.shape[0] != rows for s in given) or any(c.shape[0] < rows for c, s in zip(cols, sels) if s is None):
                        raise ValueError("the vectors of a side have one length, and a column without a vector has as many rows at least")
                    for t, (c, s) in enumerate(zip(cols, sels)):
                        d_col[t], d_sel[t] = c.data_ptr(), ptr(s)
                    setattr(d, side, rows)
            elif Desc is JoinFoldKDesc:
                if not 1 <= len(cR) <= FOLD_MAX_KEYS or len(cS) != len(cR):
                    raise ValueError("an item has 1..%d key columns a side, as many on both, not %d and %d" % (FOLD_MAX_KEYS, len(cR), len(cS)))
                d.nkeys = len(cR)
                for t, (a, b) in enumerate(zip(cR, cS)):
                    d.d_colR[t], d.d_selR, d.nR = self._cols_side(a, sR)
                    d.d_colS[t], d.d_selS, d.nS = self._cols_side(b, sS)
            else:
                d.d_colR, d.d_selR, d.nR = self._cols_side(cR, sR)
                d.d_colS, d.d_selS, d.nS = self._cols_side(cS, sS)
            d.nvalues, d.nouts = len(values), len(outs)
            for f, (w, src, col) in zip(d.values, values):
                f.d_w, f.d_src, f.d_col = ptr(w), ptr(src), ptr(col)
            mine = []
            for o, (value, (w, src, col), out) in zip(d.outs, outs):
                o.value, o.p.d_w, o.p.d_src, o.p.d_col = int(value), ptr(w), ptr(src), ptr(col)
                if out is True:
                    mine.append(at)
                    at += (d.nR + 1) // 2 * 2                    # 16-byte aligned pieces
                else:
                    if out is not None and out.numel() < d.nR:
                        raise ValueError("an output vector of %d words for %d rows" % (out.numel(), d.nR))
                    mine.append(out)
            places.append(mine)
        buf = torch.zeros(max(at, 1), dtype=torch.int64, device=self.dev)
        for d, mine in zip(arr, places):
            for o, a in zip(d.outs, mine):
                o.d_out = None if a is None else buf.data_ptr() + 8 * a if isinstance(a, int) else a.data_ptr()
        rc = getattr(self.lib, entry)(arr, n)
        if rc < 0:
            raise RuntimeError("%s failed (%d)" % (entry, rc))
        res = []
        for d, mine in zip(arr, places):
            res.append([(None if a is None else buf[a:a + d.nR] if isinstance(a, int) else a[:d.nR], d.outs[k].total) for k, a in enumerate(mine)])
        return (res, [arr[i].path for i in range(n)]) if with_info else res

    def set_fold_combine(self, on):
        """the add launches of the four table batches (join sums, folds, folds on tuple keys and on the keys of nodes), wherever
        they are issued, combine a tile's adds to one table slot in LDS and send one atomic per (tile, slot, value) (default
        on); every answer is bit for bit the same under both settings"""
        self.lib.rhj_set_fold_combine(1 if on else 0)

    def table_batch_last_combine_info(self):
        """rhj_table_batch_last_combine_info() as a dict: tiles, combined_tiles, slot_adds (all 0 with set_fold_combine off)"""
        return self.lib.rhj_table_batch_last_combine_info().contents.as_dict()

    def set_fold_resident(self, on):
        """an item of join_fold_batch_device whose table fits a workgroup's LDS (fold_resident_rule) is folded by one workgroup
        in one launch, wherever the fold batches on one key are issued (default off); it reports path 18, and every answer is
        bit for bit the same under both settings"""
        self.lib.rhj_set_fold_resident(1 if on else 0)

    def fold_resident_rule(self, nR, nS, nvalues):
        """rhj_fold_resident_rule: whether an item of these sizes is resident while set_fold_resident is on (no device needed)"""
        return bool(self.lib.rhj_fold_resident_rule(int(nR), int(nS), int(nvalues)))

    def table_batch_last_resident_info(self):
        """rhj_table_batch_last_resident_info() as a dict: resident_items, resident_launches, table_items (all 0 with
        set_fold_resident off)"""
        return self.lib.rhj_table_batch_last_resident_info().contents.as_dict()

    def set_fold_resident_keys(self, on):
        """the same for join_foldk_batch_device and join_foldn_batch_device (fold_resident_keys_rule), under a switch of its own
        (default off): a resident item reports path 19, and every answer is bit for bit the same under both settings"""
        self.lib.rhj_set_fold_resident_keys(1 if on else 0)

    def fold_resident_keys_rule(self, nR, nS, nvalues):
        """rhj_fold_resident_keys_rule: whether a tuple-key item of these sizes is resident while set_fold_resident_keys is on (no
        device needed)"""
        return bool(self.lib.rhj_fold_resident_keys_rule(int(nR), int(nS), int(nvalues)))

    def table_batch_last_resident_keys_info(self):
        """rhj_table_batch_last_resident_keys_info() as a dict: resident_items, resident_launches, table_items of the two batches
        on tuple keys (all 0 with set_fold_resident_keys off)"""
        return self.lib.rhj_table_batch_last_resident_keys_info().contents.as_dict()

    def set_query_fold(self, on):
        """query_batch_device sums the queries whose join predicates form a tree over their bindings by rounds of weighted join
        folds, without any intermediate result (default off); their rows are exact modulo 2^64"""
        self.lib.rhj_set_query_fold(1 if on else 0)

    def filter_eq2_batch_device(self, items, count_only=False, with_info=False):
        """Many two-column equalities in one call (rhj_filter_eq2_batch_device, include/rhj_inter.h): items =
        [(colA, selA, colB, selB, n), ...], int64 tensors, a vector may be None (the column's rows 0..n).  Returns
        [(indices tensor, hits), ...]: the ascending i with colA[selA[i]] == colB[selB[i]], or (None, hits) with count_only;
        the index lists are views of one allocation.  with_info: also the list of the items' path ids (9: batched)."""
        n = len(items)
        arr = (Eq2Desc * max(n, 1))()
        for d, (colA, selA, colB, selB, rows) in zip(arr, items):
            d.d_colA, d.d_selA = colA.data_ptr(), (selA.data_ptr() if selA is not None else None)
            d.d_colB, d.d_selB = colB.data_ptr(), (selB.data_ptr() if selB is not None else None)
            d.n = int(rows)
        return self._mask_batch("rhj_filter_eq2_batch_device", arr, n, count_only, with_info)

    def device_relations(self, cols):
        """(DeviceRelation array, what keeps its pointers alive) of cols[r][c]: int64 tensors, the columns of relation r"""
        arr = (DeviceRelation * max(len(cols), 1))()
        keep = []
        for d, rel in zip(arr, cols):
            p = (C.c_void_p * max(len(rel), 1))(*[c.data_ptr() if c.numel() else None for c in rel])
            keep.append(p)
            d.num_tuples, d.num_columns, d.d_columns = (rel[0].shape[0] if len(rel) else 0), len(rel), p
        return arr, keep

    def query_batch_device(self, cols, queries, with_info=False):
        """A batch of queries run level by level (rhj_query_batch_device, include/rhj_inter.h): cols[r][c] the int64 column
        tensors of relation r, queries = [(relations, joins, filters, views), ...] as query_descs() takes them.  Returns per
        query (sums, rows): the views' wrap-around sums as Python ints below 2^64 and the rows of the final result (0: the
        reference prints NULL for every view).  with_info: also rhj_query_batch_last_info() as a dict, whose attributes sum_info
        and fold_info are rhj_query_batch_last_sum_info() and rhj_query_batch_last_fold_info() as dicts."""
        rels, keep_rels = self.device_relations(cols)
        arr, keep = query_descs(queries)
        rc = self.lib.rhj_query_batch_device(rels, len(cols), arr, len(queries))
        if rc == -3:
            raise ValueError("rhj_query_batch_device refused queries %s" % [i for i in range(len(queries)) if arr[i].rc == -3])
        if rc < 0:
            raise RuntimeError("rhj_query_batch_device failed (%d)" % rc)
        del keep_rels, keep
        res = [(list(arr[i].sums[:arr[i].nviews]), arr[i].rows) for i in range(len(queries))]
        if not with_info:
            return res
        info = QueryInfo(self.lib.rhj_query_batch_last_info().contents.as_dict())
        info.sum_info = self.lib.rhj_query_batch_last_sum_info().contents.as_dict()
        info.fold_info = self.lib.rhj_query_batch_last_fold_info().contents.as_dict()
        info.foldk_info = self.lib.rhj_query_batch_last_foldk_info().contents.as_dict()
        info.fold_self_info = self.lib.rhj_query_batch_last_fold_self_info().contents.as_dict()
        info.fold_nodes_info = self.lib.rhj_query_batch_last_fold_nodes_info().contents.as_dict()
        if hasattr(self.lib, "rhj_query_batch_last_one_wait_info"):
            info.one_wait_info = self.lib.rhj_query_batch_last_one_wait_info().contents.as_dict()
        if hasattr(self.lib, "rhj_query_batch_last_products_info"):
            info.products_info = self.lib.rhj_query_batch_last_products_info().contents.as_dict()
        return res, info

    def column_stats_batch_device(self, cols, with_info=False):
        """The optimiser's statistics of many columns in one call (rhj_column_stats_batch_device, include/rhj_inter.h): cols
        int64 tensors [n] (views such as col[1:] are fine; a column may be listed twice).  Returns [(l, u, d), ...]: minimum
        and maximum as Python ints below 2^64 and the reference's distinct-value estimate as a float; (0, 0, 0.0) for an
        empty column.  with_info: also the list of the columns' path ids (11: the batched launches, 0: an empty column) and
        rhj_column_stats_batch_last_info() as a dict."""
        n = len(cols)
        arr = (ColStatsDesc * max(n, 1))()
        for d, col in zip(arr, cols):
            d.n = col.shape[0]
            d.d_col = col.data_ptr() if d.n else None
        rc = self.lib.rhj_column_stats_batch_device(arr, n)
        if rc < 0:
            raise RuntimeError("rhj_column_stats_batch_device failed (%d)" % rc)
        res = [(arr[i].l, arr[i].u, arr[i].d) for i in range(n)]
        if with_info:
            return res, [arr[i].path for i in range(n)], self.lib.rhj_column_stats_batch_last_info().contents.as_dict()
        return res

    def pairs_to_numpy(self, t):
        a = t.cpu().numpy()
        return np.ascontiguousarray(a).view(np.uint64).reshape(-1, 2).copy().view(PAIR).reshape(-1)

    # ---- host ABI: the reference's own signatures
    def RadixHashJoin(self, R, S, with_info=False):
        R = np.ascontiguousarray(R, dtype=TUPLE)
        S = np.ascontiguousarray(S, dtype=TUPLE)
        relR, relS = Relation(R.ctypes.data, len(R)), Relation(S.ctypes.data, len(S))
        res = self.lib.RadixHashJoin(C.byref(relR), C.byref(relS), None)
        null = not bool(res)
        chunks, loads = [], []
        p = res
        while p:
            n = p.contents.current_load
            loads.append(int(n))
            if n:
                buf = (C.c_char * (n * 16)).from_address(p.contents.buff)
                chunks.append(np.frombuffer(buf, dtype=PAIR).copy())
            p = p.contents.next
        total = self.lib.GetResultNum(res) if not null else 0
        if not null:
            self.lib.FreeResult(res)
        out = np.concatenate(chunks) if chunks else np.zeros(0, dtype=PAIR)
        assert total == len(out)
        return (out, {"null": null, "loads": loads}) if with_info else out

    def Filter(self, columns, rel_rows, column, op, value, sel=None, with_info=False):
        """columns: list of u64 numpy columns of ONE relation (relation_map layout);
        sel: optional row-id vector that puts the relation into the intermediate result."""
        cols = [np.ascontiguousarray(c, dtype=np.uint64) for c in columns]
        ptrs = (C.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
        rm = RelationMap(rel_rows, len(cols), ptrs, None)
        qrel = (C.c_int * 1)(0)
        fp = FilterPred(0, column, int(value), op.encode())
        table = (C.c_void_p * 1)(None)
        if sel is not None:
            sel = np.ascontiguousarray(sel, dtype=np.uint64)
            table[0] = sel.ctypes.data
        data = InterData(len(sel) if sel is not None else 0, table)
        ir = InterRes(C.pointer(data), 1, None)
        res = self.lib.Filter(C.byref(ir), C.byref(fp), C.byref(rm), qrel)
        null = not bool(res)
        chunks, loads = [], []
        p = res
        while p:
            n = p.contents.current_load
            loads.append(int(n))
            buf = (C.c_char * (n * 8)).from_address(p.contents.buff)
            chunks.append(np.frombuffer(buf, dtype=np.uint64).copy())
            p = p.contents.next
        if not null:
            self.lib.FreeResult(res)
        out = np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.uint64)
        return (out, {"null": null, "loads": loads}) if with_info else out
