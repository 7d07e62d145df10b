"""ctypes mirrors of include/fandom_search.h (structs, constants, dtypes)."""

import ctypes as C

import numpy as np

FS_OK = 0
FS_E_INVALID = -1
FS_E_NOMEM = -2
FS_E_DEVICE = -3
FS_E_CAPACITY = -4
FS_E_UNSUPPORTED = -5
FS_E_UNPROVEN = -6

FS_MODE_AUTO = 0
FS_MODE_GENERAL = 1
FS_MODE_EXACT = 2

FS_OOV_FLAG = 0x80000000

FS_ROWS_HOST = 0
FS_ROWS_DEVICE = 1
FS_ROWS_DEVICE_PACKED = 2
FS_ROWS_DEVICE_PACKED8 = 3
FS_ROWS_HEADER = 0x100
ROWS_HEADER_BYTES = 32
PACKED_ROW_BYTES = 16
PACKED8_ROW_BYTES = 8
PACKED8_MAX_SCRIPT = 1 << 18


class FsConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32),
                ("window_size", C.c_uint32),
                ("number_of_hashes", C.c_uint32),
                ("hash_dimensions", C.c_uint32),
                ("emb_dim", C.c_uint32),
                ("nearest_n", C.c_uint32),
                ("unique_filter", C.c_uint32),
                ("mode", C.c_uint32),
                ("device", C.c_int32),
                ("reserved", C.c_uint32),
                ("distance_threshold", C.c_double)]


class FsStats(C.Structure):
    _fields_ = [("windows_processed", C.c_uint64),
                ("candidates", C.c_uint64),
                ("matches", C.c_uint64),
                ("rows", C.c_uint64),
                ("scan_ms", C.c_double),
                ("total_ms", C.c_double),
                ("path", C.c_uint32),
                ("scan_launches", C.c_uint32),
                ("lsh_pending", C.c_uint32),
                ("handoff_fallbacks", C.c_uint32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class FsIndexInfo(C.Structure):
    _fields_ = [("path", C.c_uint32),
                ("proof_ok", C.c_uint32),
                ("c_max", C.c_double),
                ("cos_bound", C.c_double),
                ("norm_min", C.c_double),
                ("norm_max", C.c_double),
                ("n_script", C.c_uint64),
                ("n_windows", C.c_uint64),
                ("n_grams", C.c_uint64),
                ("filter_bytes", C.c_uint64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class FsScanShape(C.Structure):
    _fields_ = [("waves", C.c_uint32),
                ("blocks", C.c_uint32),
                ("filter_log2_words", C.c_uint32),
                ("seeds_lds_bytes", C.c_uint32),
                ("log2_buckets", C.c_uint32),
                ("log2_slots", C.c_uint32),
                ("overflow_buckets", C.c_uint32),
                ("wide_buckets", C.c_uint32),
                ("host_wire8", C.c_uint32),
                ("ids16", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]

    def as_dict(self):
        # (the launch shape; which id stream the scan reads is ScriptIndex.scan_ids16)
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name not in ("reserved", "ids16")}


# fs_row: 32 bytes
ROW_DTYPE = np.dtype([("work", np.uint32), ("fan_ix", np.uint32),
                      ("orig_ix", np.uint32), ("lev", np.uint32),
                      ("dist", np.float64), ("comb", np.float64)])
assert ROW_DTYPE.itemsize == 32


# fs_passage: 48 bytes
PASSAGE_DTYPE = np.dtype([("first", np.uint64), ("n_words", np.uint32), ("n_exact", np.uint32),
                          ("dist_sum", np.float64), ("dist_max", np.float64),
                          ("comb_sum", np.float64), ("comb_max", np.float64)])
assert PASSAGE_DTYPE.itemsize == 48

# fs_work: 56 bytes; fs_work_cell: 16 bytes
WORK_DTYPE = np.dtype([("first", np.uint64), ("n_words", np.uint32), ("fan_first", np.uint32),
                       ("fan_last", np.uint32), ("n_script_words", np.uint32),
                       ("n_passages", np.uint32), ("passage_words", np.uint32),
                       ("longest", np.uint32), ("n_groups_hit", np.uint32),
                       ("top_group", np.uint32), ("top_group_words", np.uint32),
                       ("reserved", np.uint32), ("reserved2", np.uint32)])
assert WORK_DTYPE.itemsize == 56
WORK_CELL_DTYPE = np.dtype([("work", np.uint32), ("group", np.uint32), ("n_words", np.uint32),
                            ("n_exact", np.uint32)])
assert WORK_CELL_DTYPE.itemsize == 16
FS_NONE = 0xFFFFFFFF
FS_LSH_COUNTERS = 24            # fs_index_lsh_counts
FS_WORKS_MAX_SCRIPT = 1 << 19
FS_WORKS_MAX_GROUPS = 4096

# fs_quote_word: 24 bytes; fs_quote_region: 40 bytes
QUOTE_WORD_DTYPE = np.dtype([("n_words", np.uint32), ("n_exact", np.uint32),
                             ("n_works", np.uint32), ("n_passages", np.uint32),
                             ("n_passage_works", np.uint32), ("region", np.uint32)])
assert QUOTE_WORD_DTYPE.itemsize == 24
QUOTE_REGION_DTYPE = np.dtype([("first", np.uint32), ("last", np.uint32),
                               ("n_passages", np.uint32), ("n_works", np.uint32),
                               ("n_words", np.uint32), ("n_exact", np.uint32),
                               ("peak", np.uint32), ("peak_first", np.uint32),
                               ("peak_last", np.uint32), ("reserved", np.uint32)])
assert QUOTE_REGION_DTYPE.itemsize == 40

# fs_pair_work: 16 bytes; fs_pair: 32 bytes
PAIR_WORK_DTYPE = np.dtype([("covered", np.uint32), ("partners", np.uint32),
                            ("best", np.uint32), ("best_shared", np.uint32)])
assert PAIR_WORK_DTYPE.itemsize == 16
PAIR_DTYPE = np.dtype([("a", np.uint32), ("b", np.uint32), ("shared", np.uint32),
                       ("first", np.uint32), ("last", np.uint32), ("run_first", np.uint32),
                       ("run_words", np.uint32), ("reserved", np.uint32)])
assert PAIR_DTYPE.itemsize == 32
FS_PAIRS_MAX_BYTES = 1 << 30

# fs_companion_unit: 16 bytes; fs_companion: 32 bytes
COMPANION_UNIT_DTYPE = np.dtype([("works", np.uint32), ("partners", np.uint32),
                                 ("best", np.uint32), ("best_both", np.uint32)])
assert COMPANION_UNIT_DTYPE.itemsize == 16
COMPANION_DTYPE = np.dtype([("a", np.uint32), ("b", np.uint32), ("both", np.uint32),
                            ("works_a", np.uint32), ("works_b", np.uint32),
                            ("first_work", np.uint32), ("last_work", np.uint32),
                            ("reserved", np.uint32)])
assert COMPANION_DTYPE.itemsize == 32
FS_COMPANIONS_MAX_BYTES = 1 << 30
COMPANIONS_MS_NAMES = ("incidence", "count", "place", "detail")

# fs_bundle: 64 bytes; fs_bundle_unit: 16 bytes; fs_bundle_level: 24 bytes
FS_BUNDLES_MAX_SIZE = 8
FS_BUNDLES_MAX_SETS = 1 << 22
FS_BUNDLES_MAX_BYTES = 1 << 30
FS_BUNDLES_TIMES = 32
BUNDLE_DTYPE = np.dtype([("units", np.uint32, (FS_BUNDLES_MAX_SIZE,)), ("size", np.uint32),
                         ("works", np.uint32), ("first_work", np.uint32),
                         ("extensions", np.uint32), ("closed", np.uint32),
                         ("reserved", np.uint32, (3,))])
assert BUNDLE_DTYPE.itemsize == 64
BUNDLE_UNIT_DTYPE = np.dtype([("works", np.uint32), ("sets", np.uint32), ("largest", np.uint32),
                              ("reserved", np.uint32)])
assert BUNDLE_UNIT_DTYPE.itemsize == 16
BUNDLE_LEVEL_DTYPE = np.dtype([("size", np.uint32), ("frequent", np.uint32),
                               ("candidates", np.uint64), ("closed", np.uint32),
                               ("maximal", np.uint32)])
assert BUNDLE_LEVEL_DTYPE.itemsize == 24
# fs_bundles_times: the two passes in front, four per level of size 3 .. 9, then these two
BUNDLES_LEVEL_MS_NAMES = ("join", "count", "place", "mark")

# fs_route: 64 bytes; fs_route_unit: 16 bytes; fs_route_level: 24 bytes
FS_ROUTES_MAX_LENGTH = 8
FS_ROUTES_MAX_SKIP = 63
FS_ROUTES_MAX_SETS = 1 << 22
FS_ROUTES_MAX_BYTES = 1 << 30
FS_ROUTES_TIMES = 43
ROUTE_DTYPE = np.dtype([("units", np.uint32, (FS_ROUTES_MAX_LENGTH,)), ("length", np.uint32),
                        ("works", np.uint32), ("first_work", np.uint32),
                        ("prefix_works", np.uint32), ("forward", np.uint32),
                        ("backward", np.uint32), ("closed", np.uint32),
                        ("reserved", np.uint32)])
assert ROUTE_DTYPE.itemsize == 64
ROUTE_UNIT_DTYPE = np.dtype([("works", np.uint32), ("routes", np.uint32),
                             ("longest", np.uint32), ("reserved", np.uint32)])
assert ROUTE_UNIT_DTYPE.itemsize == 16
ROUTE_LEVEL_DTYPE = np.dtype([("length", np.uint32), ("frequent", np.uint32),
                              ("candidates", np.uint64), ("closed", np.uint32),
                              ("reserved", np.uint32)])
assert ROUTE_LEVEL_DTYPE.itemsize == 24
# fs_routes_times: the pass in front, five per level of length 2 .. 9, then the records and the total
ROUTES_LEVEL_MS_NAMES = ("join", "step", "count", "place", "mark")

# fs_line, fs_line_work, fs_line_cell: 32 bytes each
LINE_DTYPE = np.dtype([("works", np.uint32), ("whole_works", np.uint32),
                       ("most_works", np.uint32), ("head_works", np.uint32),
                       ("tail_works", np.uint32), ("first_work", np.uint32),
                       ("covered_sum", np.uint64)])
assert LINE_DTYPE.itemsize == 32
LINE_WORK_DTYPE = np.dtype([("work", np.uint32), ("lines", np.uint32), ("whole_lines", np.uint32),
                            ("covered", np.uint32), ("line_words", np.uint32),
                            ("top_line", np.uint32), ("top_covered", np.uint32),
                            ("reserved", np.uint32)])
assert LINE_WORK_DTYPE.itemsize == 32
LINE_CELL_DTYPE = np.dtype([("line", np.uint32), ("work", np.uint32), ("covered", np.uint32),
                            ("first", np.uint32), ("last", np.uint32), ("runs", np.uint32),
                            ("reserved", np.uint32), ("reserved2", np.uint32)])
assert LINE_CELL_DTYPE.itemsize == 32
FS_LINES_MAX_BYTES = 1 << 30
LINES_MS_NAMES = ("tables", "walk", "total")

# fs_fragment, fs_fragment_work: 32 bytes each
FRAGMENT_DTYPE = np.dtype([("first", np.uint32), ("last", np.uint32), ("works", np.uint32),
                           ("exact_works", np.uint32), ("start_works", np.uint32),
                           ("end_works", np.uint32), ("first_work", np.uint32),
                           ("reserved", np.uint32)])
assert FRAGMENT_DTYPE.itemsize == 32
FRAGMENT_WORK_DTYPE = np.dtype([("work", np.uint32), ("runs", np.uint32), ("covered", np.uint32),
                                ("held", np.uint32), ("exact", np.uint32),
                                ("longest_first", np.uint32), ("longest_last", np.uint32),
                                ("longest_works", np.uint32)])
assert FRAGMENT_WORK_DTYPE.itemsize == 32
FS_FRAGMENTS_MAX_WORDS = 4096
FS_FRAGMENTS_MAX_BYTES = 1 << 30
FRAGMENTS_MS_NAMES = ("runs", "spread", "list", "works", "total")

# fs_digest_pick, fs_digest_work: 32 bytes each
DIGEST_PICK_DTYPE = np.dtype([("work", np.uint32), ("covered", np.uint32),
                              ("new_words", np.uint32), ("new_runs", np.uint32),
                              ("longest_first", np.uint32), ("longest_words", np.uint32),
                              ("cum_words", np.uint32), ("reserved", np.uint32)])
assert DIGEST_PICK_DTYPE.itemsize == 32
DIGEST_WORK_DTYPE = np.dtype([("work", np.uint32), ("covered", np.uint32),
                              ("pick_rank", np.uint32), ("in_picks", np.uint32),
                              ("subsumed_at", np.uint32), ("best_pick", np.uint32),
                              ("best_shared", np.uint32), ("reserved", np.uint32)])
assert DIGEST_WORK_DTYPE.itemsize == 32
FS_DIGEST_MAX_BYTES = 1 << 30
# fs_digest_times: three passes and their total in ms, then two counts
DIGEST_MS_NAMES = ("coverage", "rounds", "works", "total", "rounds_enqueued", "tiles_read")

# fs_interval_unit: 64 bytes; fs_interval_replicate: 16 bytes
INTERVAL_UNIT_DTYPE = np.dtype([("works", np.uint32), ("works_low", np.uint32),
                                ("works_median", np.uint32), ("works_high", np.uint32),
                                ("ppm", np.uint32), ("ppm_low", np.uint32),
                                ("ppm_median", np.uint32), ("ppm_high", np.uint32),
                                ("rank", np.uint32), ("next", np.uint32), ("ahead", np.uint32),
                                ("tied", np.uint32), ("behind", np.uint32),
                                ("reserved", np.uint32), ("mean_milli", np.uint64)])
assert INTERVAL_UNIT_DTYPE.itemsize == 64
INTERVAL_REPLICATE_DTYPE = np.dtype([("resampled_works", np.uint32),
                                     ("resampled_active", np.uint32),
                                     ("units_quoted", np.uint32), ("reserved", np.uint32)])
assert INTERVAL_REPLICATE_DTYPE.itemsize == 16
FS_INTERVALS_MAX_REPLICATES = 4096
FS_INTERVALS_MAX_WORKS = 1 << 28
FS_INTERVALS_MAX_BYTES = 1 << 30
INTERVALS_MS_NAMES = ("incidence", "multiplicities", "product", "statistics", "neighbours",
                      "total")

# fs_contrast_unit: 32 bytes; fs_contrast_perm: 16 bytes
CONTRAST_UNIT_DTYPE = np.dtype([("a_works", np.uint32), ("b_works", np.uint32),
                                ("ge", np.uint32), ("adj_ge", np.uint32),
                                ("statistic", np.uint64), ("d", np.int64)])
assert CONTRAST_UNIT_DTYPE.itemsize == 32
CONTRAST_PERM_DTYPE = np.dtype([("max_statistic", np.uint64), ("a_active", np.uint32),
                                ("max_unit", np.uint32)])
assert CONTRAST_PERM_DTYPE.itemsize == 16
FS_CONTRAST_MAX_PERMUTATIONS = 4096
FS_CONTRAST_MAX_WORKS = 1 << 20
FS_CONTRAST_MAX_BYTES = 1 << 30
CONTRAST_MS_NAMES = ("incidence", "selection", "product", "sweeps", "total")

# fs_trends_unit: 48 bytes; fs_trends_perm: 16 bytes
TRENDS_UNIT_DTYPE = np.dtype([("quoting", np.uint32), ("ge", np.uint32), ("adj_ge", np.uint32),
                              ("first_x", np.uint32), ("last_x", np.uint32),
                              ("reserved", np.uint32), ("offset_sum", np.uint64),
                              ("statistic", np.uint64), ("d", np.int64)])
assert TRENDS_UNIT_DTYPE.itemsize == 48
TRENDS_PERM_DTYPE = np.dtype([("max_statistic", np.uint64), ("offset_sum", np.uint32),
                              ("max_unit", np.uint32)])
assert TRENDS_PERM_DTYPE.itemsize == 16
FS_TRENDS_MAX_PERMUTATIONS = 4096
FS_TRENDS_MAX_SPAN = 1024
FS_TRENDS_MAX_WORKS = 1 << 20
FS_TRENDS_MAX_BYTES = 1 << 30
TRENDS_OUT = 0xFFFF                 # `when` of a work outside the pool
TRENDS_MS_NAMES = ("pool", "labels", "product", "sweeps", "total")

# fs_neighbour: 48 bytes; fs_neighbour_work: 32 bytes; fs_neighbour_word: 8 bytes
NEIGHBOUR_DTYPE = np.dtype([(n, np.uint32) for n in (
    "a", "b", "rank", "back_rank", "ppm", "score", "shared", "rarest", "rarest_depth",
    "rarest_weight", "run_first", "run_words")])
assert NEIGHBOUR_DTYPE.itemsize == 48
NEIGHBOUR_WORK_DTYPE = np.dtype([(n, np.uint32) for n in (
    "covered", "own", "candidates", "listed", "listed_by", "mutual", "nearest", "nearest_ppm")])
assert NEIGHBOUR_WORK_DTYPE.itemsize == 32
NEIGHBOUR_WORD_DTYPE = np.dtype([("depth", np.uint32), ("weight", np.uint32)])
assert NEIGHBOUR_WORD_DTYPE.itemsize == 8
FS_NEIGHBOURS_RARITY, FS_NEIGHBOURS_FLAT = 0, 1
FS_NEIGHBOURS_MAX_TOP = 32
FS_NEIGHBOURS_MAX_BYTES = 1 << 30
NEIGHBOURS_MS_NAMES = ("coverage", "weights", "product", "place", "detail", "total")

# fs_misquote, fs_misquote_pair and fs_misquote_work: 32 bytes each
MISQUOTE_DTYPE = np.dtype([(n, np.uint32) for n in (
    "orig_ix", "spell", "records", "works", "readers", "telling", "weight", "first_work")])
assert MISQUOTE_DTYPE.itemsize == 32
MISQUOTE_PAIR_DTYPE = np.dtype([(n, np.uint32) for n in (
    "a", "b", "shared", "score", "a_on_common", "b_on_common", "strongest",
    "strongest_weight")])
assert MISQUOTE_PAIR_DTYPE.itemsize == 32
MISQUOTE_WORK_DTYPE = np.dtype([(n, np.uint32) for n in (
    "passage_records", "departures", "misquotes", "telling", "singular", "partners", "closest",
    "closest_score")])
assert MISQUOTE_WORK_DTYPE.itemsize == 32
FS_MISQUOTES_RARITY, FS_MISQUOTES_FLAT = 0, 1
FS_MISQUOTES_SLOT_BYTES = 32
FS_MISQUOTES_RECORD_SLOT_BYTES = 40
FS_MISQUOTES_MAX_BYTES = 1 << 30
FS_MISQUOTES_MAX_ROWS = 1 << 27
MISQUOTES_MS_NAMES = ("passages", "cells", "number", "postings", "expand", "place", "detail",
                      "total")

# fs_saturation_point: 64 bytes; fs_saturation_perm and fs_saturation_summary: 16 bytes
SATURATION_POINT_DTYPE = np.dtype([("units_low", np.uint32), ("units_median", np.uint32),
                                   ("units_high", np.uint32), ("units_min", np.uint32),
                                   ("units_max", np.uint32), ("works_low", np.uint32),
                                   ("works_median", np.uint32), ("works_high", np.uint32),
                                   ("units_sum", np.uint64), ("works_sum", np.uint64),
                                   ("reserved0", np.uint64), ("reserved1", np.uint64)])
assert SATURATION_POINT_DTYPE.itemsize == 64
SATURATION_PERM_DTYPE = np.dtype([("half_at", np.uint32), ("ninety_at", np.uint32),
                                  ("all_at", np.uint32), ("reserved", np.uint32)])
assert SATURATION_PERM_DTYPE.itemsize == 16
SATURATION_SUMMARY_DTYPE = np.dtype([("n_active", np.uint32), ("units_quoted", np.uint32),
                                     ("singletons", np.uint32), ("doubletons", np.uint32)])
assert SATURATION_SUMMARY_DTYPE.itemsize == 16
FS_SATURATION_MAX_PERMUTATIONS = 4096
FS_SATURATION_MAX_POINTS = 1024
FS_SATURATION_MAX_WORKS = 1 << 28
FS_SATURATION_MAX_BYTES = 1 << 30
# fs_saturation_times: six passes and their total in ms, then the product's source and its shares of k and of the orders
SATURATION_MS_NAMES = ("incidence", "sizes", "times", "product", "curve", "points", "total",
                       "table", "ksplit", "osplit")

# fs_transition_unit: 40 bytes; fs_transition: 32 bytes
TRANSITION_UNIT_DTYPE = np.dtype([("passages", np.uint32), ("works", np.uint32),
                                  ("starts", np.uint32), ("ends", np.uint32),
                                  ("steps_out", np.uint32), ("steps_in", np.uint32),
                                  ("successors", np.uint32), ("predecessors", np.uint32),
                                  ("best_next", np.uint32), ("best_steps", np.uint32)])
assert TRANSITION_UNIT_DTYPE.itemsize == 40
TRANSITION_DTYPE = np.dtype([("a", np.uint32), ("b", np.uint32), ("steps", np.uint32),
                             ("advances", np.uint32), ("works", np.uint32),
                             ("first_work", np.uint32), ("steps_out_a", np.uint32),
                             ("steps_in_b", np.uint32)])
assert TRANSITION_DTYPE.itemsize == 32
FS_TRANSITIONS_DENSE = 64
TRANSITIONS_MS_NAMES = ("sequence", "count", "keep", "place", "total")


# fs_source_cols: 40 bytes; fs_source_passage: 80; fs_source_work: 56; fs_source_script and
# fs_source_pair: 48 each
class FsSourceCols(C.Structure):
    _fields_ = [("work", C.POINTER(C.c_uint32)),
                ("fan_ix", C.POINTER(C.c_uint32)),
                ("orig_ix", C.POINTER(C.c_uint32)),
                ("comb", C.POINTER(C.c_double)),
                ("n", C.c_uint64)]


assert C.sizeof(FsSourceCols) == 40
SOURCE_PASSAGE_DTYPE = np.dtype([("script", np.uint32), ("work", np.uint32),
                                 ("first", np.uint32), ("n_words", np.uint32),
                                 ("n_exact", np.uint32), ("fan_first", np.uint32),
                                 ("fan_last", np.uint32), ("orig_first", np.uint32),
                                 ("orig_last", np.uint32), ("rivals", np.uint32),
                                 ("rival_scripts", np.uint32), ("outcome", np.uint32),
                                 ("best_rival", np.uint32), ("best_rival_words", np.uint32),
                                 ("best_rival_fan_first", np.uint32), ("reserved", np.uint32),
                                 ("contested_words", np.uint64), ("sole_words", np.uint64)])
assert SOURCE_PASSAGE_DTYPE.itemsize == 80
SOURCE_WORK_DTYPE = np.dtype([("work", np.uint32), ("script", np.uint32),
                              ("passages", np.uint32), ("alone", np.uint32), ("won", np.uint32),
                              ("lost", np.uint32), ("work_scripts", np.uint32),
                              ("primary", np.uint32), ("covered_words", np.uint64),
                              ("contested_words", np.uint64), ("sole_words", np.uint64)])
assert SOURCE_WORK_DTYPE.itemsize == 56
SOURCE_SCRIPT_DTYPE = np.dtype([("works", np.uint32), ("passages", np.uint32),
                                ("alone", np.uint32), ("won", np.uint32), ("lost", np.uint32),
                                ("primary_works", np.uint32), ("covered_words", np.uint64),
                                ("contested_words", np.uint64), ("sole_words", np.uint64)])
assert SOURCE_SCRIPT_DTYPE.itemsize == 48
SOURCE_PAIR_DTYPE = np.dtype([("a", np.uint32), ("b", np.uint32), ("works_both", np.uint32),
                              ("reserved", np.uint32), ("contests", np.uint64),
                              ("shared_words", np.uint64), ("a_wins", np.uint64),
                              ("b_wins", np.uint64)])
assert SOURCE_PAIR_DTYPE.itemsize == 48
FS_SOURCES_MAX_FILES = 64
FS_SOURCES_MAX_BYTES = 1 << 30
FS_SOURCE_ALONE, FS_SOURCE_WON, FS_SOURCE_LOST = 0, 1, 2
SOURCES_MS_NAMES = ("passages", "contest", "union", "rollups", "total")

# fs_cluster_work: 32 bytes; fs_cluster: 48 bytes
CLUSTER_WORK_DTYPE = np.dtype([("covered", np.uint32), ("root", np.uint32), ("size", np.uint32),
                               ("cluster", np.uint32), ("links", np.uint32), ("best", np.uint32),
                               ("best_shared", np.uint32), ("reserved", np.uint32)])
assert CLUSTER_WORK_DTYPE.itemsize == 32
CLUSTER_DTYPE = np.dtype([("root", np.uint32), ("n_works", np.uint32), ("n_links", np.uint32),
                          ("hub", np.uint32), ("hub_links", np.uint32), ("covered", np.uint32),
                          ("common", np.uint32), ("peak", np.uint32), ("peak_first", np.uint32),
                          ("run_first", np.uint32), ("run_words", np.uint32),
                          ("reserved", np.uint32)])
assert CLUSTER_DTYPE.itemsize == 48
FS_CLUSTERS_MAX_BYTES = 1 << 30

# fs_tree_merge: 64 bytes; fs_tree_work and fs_tree_level: 32 bytes
TREE_MERGE_DTYPE = np.dtype([(n, np.uint32) for n in (
    "a", "b", "level", "shared", "a_covered", "b_covered", "left", "right", "left_works",
    "right_works", "works", "first_work", "tree", "run_first", "run_words", "reserved")])
assert TREE_MERGE_DTYPE.itemsize == 64
TREE_WORK_DTYPE = np.dtype([(n, np.uint32) for n in (
    "covered", "tree", "tree_works", "edges", "joined_merge", "joined_level", "best", "leaf")])
assert TREE_WORK_DTYPE.itemsize == 32
TREE_LEVEL_DTYPE = np.dtype([(n, np.uint32) for n in (
    "level", "merges", "merges_above", "families", "largest", "joined", "singles", "reserved")])
assert TREE_LEVEL_DTYPE.itemsize == 32
FS_TREE_JACCARD, FS_TREE_SHARED = 0, 1
TREE_MEASURES = ("jaccard", "shared")
FS_TREE_MAX_BYTES = 1 << 30
FS_TREE_ROW_BYTES = 60
FS_TREE_MAX_ROUNDS = 40
TREE_MS_NAMES = ("cover", "flatten", "best", "choose", "hook", "detail", "replay", "total",
                 "rounds")

# fs_group: 64 bytes; fs_group_cell: 24 bytes; fs_group_word: 16 bytes
GROUP_DTYPE = np.dtype([("n_works", np.uint32), ("n_passage_works", np.uint32),
                        ("n_words", np.uint32), ("n_exact", np.uint32),
                        ("n_passages", np.uint32), ("passage_words", np.uint32),
                        ("longest", np.uint32), ("covered", np.uint32), ("peak", np.uint32),
                        ("peak_first", np.uint32), ("top_label", np.uint32),
                        ("top_label_words", np.uint32), ("n_cells", np.uint32),
                        ("n_word_rows", np.uint32), ("reserved", np.uint32),
                        ("reserved2", np.uint32)])
assert GROUP_DTYPE.itemsize == 64
GROUP_CELL_DTYPE = np.dtype([("group", np.uint32), ("label", np.uint32), ("n_words", np.uint32),
                             ("n_exact", np.uint32), ("n_works", np.uint32),
                             ("reserved", np.uint32)])
assert GROUP_CELL_DTYPE.itemsize == 24
GROUP_WORD_DTYPE = np.dtype([("group", np.uint32), ("orig_ix", np.uint32),
                             ("n_works", np.uint32), ("reserved", np.uint32)])
assert GROUP_WORD_DTYPE.itemsize == 16
FS_GROUPS_MAX_BYTES = 1 << 30

# fs_variant_cell, fs_variant_word: 16 bytes each
VARIANT_CELL_DTYPE = np.dtype([("orig_ix", np.uint32), ("spell", np.uint32),
                               ("n_records", np.uint32), ("n_works", np.uint32)])
assert VARIANT_CELL_DTYPE.itemsize == 16
VARIANT_WORD_DTYPE = np.dtype([("n_records", np.uint32), ("n_spellings", np.uint32),
                               ("n_works", np.uint32), ("first_cell", np.uint32)])
assert VARIANT_WORD_DTYPE.itemsize == 16

# fs_reading 40 bytes, fs_reading_span 24
READING_DTYPE = np.dtype([("first", np.uint64), ("orig_first", np.uint32),
                          ("orig_last", np.uint32), ("n_words", np.uint32),
                          ("n_passages", np.uint32), ("n_works", np.uint32), ("span", np.uint32),
                          ("rank", np.uint32), ("reserved", np.uint32)])
assert READING_DTYPE.itemsize == 40
READING_SPAN_DTYPE = np.dtype([("orig_first", np.uint32), ("orig_last", np.uint32),
                               ("n_passages", np.uint32), ("n_works", np.uint32),
                               ("n_readings", np.uint32), ("first_reading", np.uint32)])
assert READING_SPAN_DTYPE.itemsize == 24
FS_READINGS_MAX_BYTES = 1 << 30
FS_READINGS_SLOT_BYTES = 64
READINGS_MS_NAMES = ("passages", "tables", "spans", "readings", "copy_out", "total")

# fs_fanon_work 40 bytes, fs_fanon_gram 16, fs_fanon_passage 24, fs_fanon_phrase 32
FANON_WORK_DTYPE = np.dtype([("n_tokens", np.uint32), ("n_positions", np.uint32),
                             ("shared_positions", np.uint32), ("canon_positions", np.uint32),
                             ("common_positions", np.uint32), ("n_passages", np.uint32),
                             ("shared_tokens", np.uint32), ("canon_tokens", np.uint32),
                             ("longest_start", np.uint32), ("longest_tokens", np.uint32)])
assert FANON_WORK_DTYPE.itemsize == 40
FANON_GRAM_DTYPE = np.dtype([("work", np.uint32), ("start", np.uint32), ("works", np.uint32),
                             ("occurrences", np.uint32)])
assert FANON_GRAM_DTYPE.itemsize == 16
FANON_PASSAGE_DTYPE = np.dtype([("work", np.uint32), ("start", np.uint32),
                                ("n_tokens", np.uint32), ("phrase", np.uint32),
                                ("least", np.uint32), ("most", np.uint32)])
assert FANON_PASSAGE_DTYPE.itemsize == 24
FANON_PHRASE_DTYPE = np.dtype([("work", np.uint32), ("start", np.uint32),
                               ("n_tokens", np.uint32), ("n_passages", np.uint32),
                               ("n_works", np.uint32), ("least", np.uint32), ("most", np.uint32),
                               ("reserved", np.uint32)])
assert FANON_PHRASE_DTYPE.itemsize == 32
FS_FANON_NO_ID = 0xFFFFFFFF
FS_FANON_MIN_LENGTH = 2
FS_FANON_MAX_LENGTH = 32
FS_FANON_TILE = 256
FS_FANON_MAX_BYTES = 8 << 30
FANON_MS_NAMES = ("insert", "flag", "phrases", "place", "works", "copy_out", "total")

# fs_retelling 40 bytes, fs_retelling_passage 48
RETELLING_DTYPE = np.dtype([("n_passages", np.uint32), ("passage_words", np.uint32),
                            ("chain_passages", np.uint32), ("chain_words", np.uint32),
                            ("chain_first", np.uint32), ("chain_last", np.uint32),
                            ("orig_first", np.uint32), ("orig_last", np.uint32),
                            ("chain_script_words", np.uint32), ("n_descents", np.uint32)])
assert RETELLING_DTYPE.itemsize == 40
RETELLING_PASSAGE_DTYPE = np.dtype([("first", np.uint64), ("n_words", np.uint32),
                                    ("work", np.uint32), ("fan_first", np.uint32),
                                    ("fan_last", np.uint32), ("orig_first", np.uint32),
                                    ("orig_last", np.uint32), ("best", np.uint32),
                                    ("prev", np.uint32), ("depth", np.uint32),
                                    ("chain_pos", np.uint32)])
assert RETELLING_PASSAGE_DTYPE.itemsize == 48
RETELLINGS_MS_NAMES = ("passages", "bins", "chains", "trace", "write", "total")

# fs_alignment 56 bytes
ALIGNMENT_DTYPE = np.dtype([("first", np.uint64), ("last", np.uint64), ("n_words", np.uint32),
                            ("n_exact", np.uint32), ("score", np.uint32),
                            ("fan_skipped", np.uint32), ("orig_skipped", np.uint32),
                            ("pieces", np.uint32), ("tree_records", np.uint32),
                            ("reserved", np.uint32), ("path_at", np.uint64)])
assert ALIGNMENT_DTYPE.itemsize == 56
FS_ALIGNMENTS_MAX_REACH = 63
FS_ALIGNMENTS_MAX_MATCH = 16
FS_ALIGNMENTS_MAX_GAP = 16
ALIGNMENTS_MS_NAMES = ("segments", "bins", "chain", "keep", "trace", "total")

# fs_matrix_ngram 8 bytes
FS_MATRIX_MAX_BYTES = 1 << 30
MATRIX_NGRAM_DTYPE = np.dtype([("work", np.uint32), ("start", np.uint32)])
assert MATRIX_NGRAM_DTYPE.itemsize == 8
MATRIX_MS_NAMES = ("runs", "spans", "counter", "pick", "place", "total")

# the match CSV reader (fs_matches_*): fs_match_ix 64 bytes, fs_match_defer 8, fs_matches_info 96
FS_MATCH_FIELDS = 12
FS_MATCHES_PARSED = 0
FS_MATCHES_DEFERRED = 1
FS_MATCHES_OUTSIDE = 2
FS_MATCH_BAD_NUL, FS_MATCH_BAD_OPEN, FS_MATCH_BAD_CLOSE, FS_MATCH_BAD_CR = 1, 2, 4, 8
FS_MATCH_BAD_FIELDS, FS_MATCH_BAD_INT, FS_MATCH_BAD_UTF8, FS_MATCH_BAD_ROW = 16, 32, 64, 128
FS_MATCH_BAD_DEFER = 256
MATCH_IX_DTYPE = np.dtype([("start", np.uint64), ("end", np.uint32, (FS_MATCH_FIELDS,)),
                           ("quoted", np.uint32), ("head", np.uint32)])
assert MATCH_IX_DTYPE.itemsize == 64
MATCH_DEFER_DTYPE = np.dtype([("row", np.uint32), ("col", np.uint32)])
assert MATCH_DEFER_DTYPE.itemsize == 8
FS_DEC_SURE = 0
FS_DEC_NOT_MINE = 1


class FsMatchesInfo(C.Structure):
    _fields_ = [("n_rows", C.c_uint64),
                ("n_deferred", C.c_uint64),
                ("status", C.c_uint32),
                ("reason", C.c_uint32),
                ("has_header", C.c_uint32),
                ("reserved", C.c_uint32),
                ("ms", C.c_double * 8)]


MATCHES_MS_NAMES = ("upload", "parity", "classify", "place", "header", "rows", "device_total")
INTERN_MS_NAMES = ("clear", "insert", "number", "copy", "device_total")   # fs_matches_intern_times


def default_unique_filter():
    """Whether a query's bucket contents go through NearPy's UniqueFilter before the
    distances are taken.  OFF by default: the reference calls `engine.neighbours(row)`
    with no arguments (/root/reference/search.py:178), and NearPy 1.0.0 -- the release pip
    installed when the reference was written; requirements.txt pins none -- applies fetch
    filters only when they are passed to neighbours() itself (`if fetch_vector_filters:`
    on the ARGUMENT; the engine's own default [UniqueFilter()] is never consulted there),
    so a script window found under k of the 15 hashes comes back k times and takes k of
    NearestFilter(10)'s places.  NearPy 0.2.x applied the engine's filter:
    FANDOM_SEARCH_UNIQUE_FILTER=1 (or `ao3.py search --unique-filter 1`) gives that."""
    import os
    return os.environ.get("FANDOM_SEARCH_UNIQUE_FILTER", "0").strip() not in ("", "0", "false", "no", "off")


def make_config(window_size=6, number_of_hashes=15, hash_dimensions=14,
                distance_threshold=0.1, emb_dim=300, nearest_n=10,
                unique_filter=None, mode=FS_MODE_AUTO, device=0):
    """Defaults are the keyword defaults of the reference's analyze()
    (/root/reference/search.py:336-341) and what NearPy's Engine does with the defaults
    the reference leaves it (unique_filter: default_unique_filter())."""
    if unique_filter is None:
        unique_filter = default_unique_filter()
    cfg = FsConfig()
    cfg.struct_size = C.sizeof(FsConfig)
    cfg.window_size = window_size
    cfg.number_of_hashes = number_of_hashes
    cfg.hash_dimensions = hash_dimensions
    cfg.emb_dim = emb_dim
    cfg.nearest_n = nearest_n
    cfg.unique_filter = 1 if unique_filter else 0
    cfg.mode = mode
    cfg.device = device
    cfg.distance_threshold = distance_threshold
    return cfg


def ptr(arr, ctype):
    """Typed pointer to a C-contiguous numpy array (None -> NULL)."""
    if arr is None:
        return None
    return arr.ctypes.data_as(C.POINTER(ctype))


def as_u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def as_u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)
