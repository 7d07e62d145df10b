"""Loader of libfandomsearch_hip.so (the C ABI of include/fandom_search.h).

There is no CPU fallback: if the library is missing or cannot be loaded the
import of anything that needs it fails with a clear error.
"""

import ctypes as C
import os
import sys
import subprocess

from . import abi

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libfandomsearch_hip.so"
_LIB = None

SYMBOLS = ("fs_version", "fs_strerror", "fs_last_error", "fs_index_create",
           "fs_index_info_get", "fs_index_destroy", "fs_corpus_create",
           "fs_corpus_destroy", "fs_corpus_view", "fs_search_corpus", "fs_search",
           "fs_scan_benchmark", "fs_corpus_update_begin", "fs_corpus_update_end",
           "fs_host_alloc", "fs_host_free", "fs_rows_unpack", "fs_rows_unpack8",
           "fs_reuse_histogram", "fs_reuse_histogram_rows", "fs_passages", "fs_passages_rows",
           "fs_works", "fs_works_rows", "fs_quotes", "fs_quotes_rows", "fs_variants",
           "fs_readings", "fs_readings_times",
           "fs_fanon", "fs_fanon_dev", "fs_fanon_times",
           "fs_retellings", "fs_retellings_rows", "fs_retellings_times",
           "fs_alignments", "fs_alignments_rows", "fs_alignments_times",
           "fs_pairs", "fs_pairs_rows", "fs_pairs_times",
           "fs_companions", "fs_companions_rows", "fs_companions_times",
           "fs_bundles", "fs_bundles_rows", "fs_bundles_times",
           "fs_routes", "fs_routes_rows", "fs_routes_times",
           "fs_lines", "fs_lines_rows", "fs_lines_times",
           "fs_fragments", "fs_fragments_rows", "fs_fragments_times",
           "fs_digest", "fs_digest_rows", "fs_digest_times",
           "fs_intervals", "fs_intervals_rows", "fs_intervals_times",
           "fs_contrast", "fs_contrast_rows", "fs_contrast_times", "fs_contrast_isqrt",
           "fs_trends", "fs_trends_rows", "fs_trends_times",
           "fs_neighbours", "fs_neighbours_rows", "fs_neighbours_times",
           "fs_misquotes", "fs_misquotes_times",
           "fs_saturation", "fs_saturation_rows", "fs_saturation_times", "fs_saturation_bucket",
           "fs_transitions", "fs_transitions_rows", "fs_transitions_times",
           "fs_sources", "fs_sources_times",
           "fs_matrix", "fs_matrix_rows", "fs_matrix_times",
           "fs_clusters", "fs_clusters_rows", "fs_clusters_times",
           "fs_tree", "fs_tree_rows", "fs_tree_times",
           "fs_groups", "fs_groups_rows", "fs_groups_times",
           "fs_search_corpus_begin", "fs_search_corpus_end", "fs_index_set_scan_timing",
           "fs_index_reload_switches", "fs_search_kernel_name", "fs_index_scan_shape", "fs_debug_stamps",
           "fs_debug_ids16_window",
           "fs_search_profile", "fs_index_component_sizes", "fs_index_share_info", "fs_index_share_counts", "fs_index_lsh_counts",
           "fs_stream_floor",
           "fs_textenc_create", "fs_textenc_destroy", "fs_textenc_add", "fs_textenc_encode_files",
           "fs_textenc_encode_files_vec",
           "fs_csvw_create", "fs_csvw_destroy", "fs_csvw_set_script", "fs_csvw_add_strings", "fs_csvw_strings",
           "fs_csvw_format",
           "fs_matches_open", "fs_matches_read", "fs_matches_labels", "fs_matches_close",
           "fs_matches_intern", "fs_matches_intern_times",
           "fs_matches_parse_double")


# the commands with an fs_<name>_times(double *ms) beside their entry points
TIMED = ("readings", "fanon", "retellings", "alignments", "pairs", "companions", "bundles", "routes", "lines", "fragments", "digest", "intervals", "contrast", "trends", "neighbours", "misquotes", "saturation", "transitions", "sources", "matrix",
         "clusters", "tree", "groups")


class FsError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        msg = "%s failed: %d" % (where, code)
        if detail:
            msg += " (%s)" % detail
        RuntimeError.__init__(self, msg)


PRELOAD_TORCH = True    # see load()


def lib_path():
    # FS_LIB_FILE: another build of the same library (A/B measurements of two builds
    # in one GPU session); it must sit next to the regular one
    return os.path.join(_PKG, os.path.basename(os.environ.get("FS_LIB_FILE", LIB_NAME)))


def source_hash():
    """Identifies the kernels a measurement belongs to: SHA-256 (first 16 hex digits) over
    the library's sources (csrc/*.hip, csrc/*.h, include/fandom_search.h), which travel
    with the built .so.  Artifacts under profiles/ carry it, and bench.py refuses a
    traffic figure whose stamp differs from the sources it runs (git is not available
    where the measurements are made)."""
    import hashlib
    h = hashlib.sha256()
    src = os.path.join(_PKG, "csrc")
    files = sorted(f for f in os.listdir(src) if f.endswith((".hip", ".h")))
    paths = [os.path.join(src, f) for f in files]
    paths.append(os.path.join(os.path.dirname(_PKG), "include", "fandom_search.h"))
    for path in paths:
        h.update(os.path.basename(path).encode())
        with open(path, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def build(verbose=False):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles
    without a GPU)."""
    cmd = ["make", "-C", os.path.join(_PKG, "csrc")]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    return lib_path()


def load():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            "%s is not built; run `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C fandom_search_amd/csrc`. There is no CPU "
            "fallback for the search path." % path)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so
    # (SONAME libamdhip64.so.7).  Loaded first, it satisfies this library's
    # DT_NEEDED libamdhip64.so.7 as well; loaded second, it would come in as a second
    # runtime next to /opt/rocm's (two sets of queues and contexts, and torch can then
    # fail with "No HIP GPUs are available" late in a long process).
    # PRELOAD_TORCH = False (the single-process command line, which never imports torch:
    # its start-up costs a second) loads the library against /opt/rocm's runtime alone.
    if PRELOAD_TORCH or "torch" in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(path)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L.fs_version.restype = C.c_int
    L.fs_strerror.restype = C.c_char_p
    L.fs_strerror.argtypes = [C.c_int]
    L.fs_last_error.restype = C.c_char_p
    L.fs_index_create.restype = C.c_int
    L.fs_index_create.argtypes = [
        C.POINTER(abi.FsConfig), u32p, u32p, u64p, C.c_uint64,
        C.POINTER(C.c_float), C.c_uint64, C.POINTER(C.c_double),
        C.POINTER(C.c_void_p)]
    L.fs_index_info_get.restype = C.c_int
    L.fs_index_info_get.argtypes = [C.c_void_p, C.POINTER(abi.FsIndexInfo)]
    L.fs_index_destroy.restype = None
    L.fs_index_destroy.argtypes = [C.c_void_p]
    L.fs_corpus_create.restype = C.c_int
    L.fs_corpus_create.argtypes = [
        C.c_void_p, u32p, u32p, u64p, C.c_uint64, u32p, u64p, C.c_uint64,
        C.POINTER(C.c_void_p)]
    L.fs_corpus_view.restype = C.c_int
    L.fs_corpus_view.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    L.fs_corpus_destroy.restype = None
    L.fs_corpus_destroy.argtypes = [C.c_void_p]
    L.fs_search_corpus.restype = C.c_int
    L.fs_search_corpus.argtypes = [
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, u64p,
        C.POINTER(abi.FsStats)]
    L.fs_search.restype = C.c_int
    L.fs_search.argtypes = [
        C.c_void_p, u32p, u32p, u64p, C.c_uint64, u32p, u64p, C.c_uint64,
        C.c_void_p, C.c_uint64, u64p, C.POINTER(abi.FsStats)]
    L.fs_corpus_update_begin.restype = C.c_int
    L.fs_corpus_update_begin.argtypes = [C.c_void_p, u32p, u32p, u64p, C.c_uint64]
    L.fs_corpus_update_end.restype = C.c_int
    L.fs_corpus_update_end.argtypes = [C.c_void_p]
    L.fs_host_alloc.restype = C.c_int
    L.fs_host_alloc.argtypes = [C.c_uint64, C.POINTER(C.c_void_p)]
    L.fs_host_free.restype = None
    L.fs_host_free.argtypes = [C.c_void_p]
    L.fs_rows_unpack.restype = C.c_int
    L.fs_rows_unpack.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.fs_rows_unpack8.restype = C.c_int
    L.fs_rows_unpack8.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                  C.c_void_p]
    L.fs_reuse_histogram.restype = C.c_int
    L.fs_reuse_histogram.argtypes = [C.c_int, u32p, C.POINTER(C.c_double), C.c_uint64, C.c_uint64,
                                     C.POINTER(C.c_double), C.c_uint32, u32p]
    L.fs_reuse_histogram_rows.restype = C.c_int
    L.fs_reuse_histogram_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64,
                                          C.POINTER(C.c_double), C.c_uint32, C.c_void_p]
    L.fs_passages.restype = C.c_int
    L.fs_passages.argtypes = [C.c_int, u32p, u32p, u32p, C.POINTER(C.c_double),
                              C.POINTER(C.c_double), C.c_uint64, C.c_uint32, C.c_uint32,
                              C.c_void_p, C.c_uint64, u64p]
    L.fs_passages_rows.restype = C.c_int
    L.fs_passages_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                   C.c_void_p, C.c_uint64, u64p]
    L.fs_works.restype = C.c_int
    L.fs_works.argtypes = [C.c_int, u32p, u32p, u32p, C.POINTER(C.c_double), C.c_uint64,
                           C.c_uint32, C.c_uint32, u32p, C.c_uint32, C.c_uint32, C.c_uint32,
                           C.POINTER(C.c_double), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                           C.c_uint64, u64p]
    L.fs_works_rows.restype = C.c_int
    L.fs_works_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, u32p, C.c_uint32,
                                C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.c_uint32,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.fs_quotes.restype = C.c_int
    L.fs_quotes.argtypes = [C.c_int, u32p, u32p, u32p, C.POINTER(C.c_double), C.c_uint64,
                            C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                            C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.fs_quotes_rows.restype = C.c_int
    L.fs_quotes_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                 C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.fs_pairs.restype = C.c_int
    L.fs_pairs.argtypes = [C.c_int, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                           C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                           u64p]
    L.fs_pairs_rows.restype = C.c_int
    L.fs_pairs_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.fs_companions.restype = C.c_int
    L.fs_companions.argtypes = [C.c_int, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                                u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.fs_companions_rows.restype = C.c_int
    L.fs_companions_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.fs_bundles.restype = C.c_int
    L.fs_bundles.argtypes = [C.c_int, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                             u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.fs_bundles_rows.restype = C.c_int
    L.fs_bundles_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                  C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.fs_routes.restype = C.c_int
    L.fs_routes.argtypes = [C.c_int, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                            u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                            C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.fs_routes_rows.restype = C.c_int
    L.fs_routes_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                 C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                 C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                 u64p]
    L.fs_lines.restype = C.c_int
    L.fs_lines.argtypes = [C.c_int, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32, u32p,
                           C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                           C.c_uint64, u64p, C.c_void_p, C.c_uint64, u64p]
    L.fs_lines_rows.restype = C.c_int
    L.fs_lines_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.c_uint64, u64p]
    L.fs_fragments.restype = C.c_int
    L.fs_fragments.argtypes = [C.c_int, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                               C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                               C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.c_uint64, u64p]
    L.fs_fragments_rows.restype = C.c_int
    L.fs_fragments_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                    C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                    C.c_uint64, u64p, C.c_void_p, C.c_uint64, u64p]
    L.fs_digest.restype = C.c_int
    L.fs_digest.argtypes = [C.c_int, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                            C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                            C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.c_uint64, u64p, u64p]
    L.fs_digest_rows.restype = C.c_int
    L.fs_digest_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                 C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                 C.c_uint64, u64p, C.c_void_p, C.c_uint64, u64p, u64p]
    L.fs_intervals.restype = C.c_int
    L.fs_intervals.argtypes = [C.c_int, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                               u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                               C.c_uint32, C.c_void_p, C.c_void_p]
    L.fs_intervals_rows.restype = C.c_int
    L.fs_intervals_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                    C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                    C.c_uint32, C.c_void_p, C.c_void_p]
    L.fs_contrast.restype = C.c_int
    L.fs_contrast.argtypes = [C.c_int, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                              u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                              C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                              C.c_void_p]
    L.fs_contrast_rows.restype = C.c_int
    L.fs_contrast_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                   C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                   C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
    L.fs_contrast_isqrt.restype = C.c_uint64
    L.fs_contrast_isqrt.argtypes = [C.c_uint64]
    L.fs_trends.restype = C.c_int
    L.fs_trends.argtypes = [C.c_int, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                            u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                            C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fs_trends_rows.restype = C.c_int
    L.fs_trends_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                 C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                 C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
    L.fs_neighbours.restype = C.c_int
    L.fs_neighbours.argtypes = [C.c_int, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                                C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.fs_neighbours_rows.restype = C.c_int
    L.fs_neighbours_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.fs_misquotes.restype = C.c_int
    L.fs_misquotes.argtypes = [C.c_int, u32p, u32p, u32p, u32p, u32p, C.c_uint64, C.c_uint32,
                               C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                               C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                               C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.c_uint64, u64p]
    L.fs_saturation.restype = C.c_int
    L.fs_saturation.argtypes = [C.c_int, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                                u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p]
    L.fs_saturation_rows.restype = C.c_int
    L.fs_saturation_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]
    L.fs_saturation_bucket.restype = C.c_uint32
    L.fs_saturation_bucket.argtypes = [C.c_uint32, C.c_uint32]
    L.fs_transitions.restype = C.c_int
    L.fs_transitions.argtypes = [C.c_int, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                                 u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                 C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.fs_transitions_rows.restype = C.c_int
    L.fs_transitions_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                      C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                                      u64p]
    L.fs_sources.restype = C.c_int
    L.fs_sources.argtypes = [C.c_int, C.POINTER(abi.FsSourceCols), C.c_uint32, C.c_uint32,
                             C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, u64p, C.c_void_p,
                             C.c_uint64, u64p, C.c_void_p, C.c_void_p]
    L.fs_clusters.restype = C.c_int
    L.fs_clusters.argtypes = [C.c_int, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                              C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                              C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.fs_clusters_rows.restype = C.c_int
    L.fs_clusters_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                   C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                   C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.fs_tree.restype = C.c_int
    L.fs_tree.argtypes = [C.c_int, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                          C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                          C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.c_uint64, u64p]
    L.fs_tree_rows.restype = C.c_int
    L.fs_tree_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                               C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                               C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.c_uint64, u64p]
    L.fs_groups.restype = C.c_int
    L.fs_groups.argtypes = [C.c_int, u32p, u32p, u32p, C.POINTER(C.c_uint8), C.c_uint64,
                            C.c_uint32, C.c_uint32, u64p, u32p, C.c_uint32, u32p, C.c_uint32,
                            C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                            C.c_uint64, u64p, C.c_void_p, C.c_uint64, u64p]
    L.fs_groups_rows.restype = C.c_int
    L.fs_groups_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, u64p, u32p,
                                 C.c_uint32, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                 C.c_void_p, C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.c_uint64,
                                 u64p]
    L.fs_matches_open.restype = C.c_int
    L.fs_matches_open.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p),
                                  C.POINTER(abi.FsMatchesInfo)]
    L.fs_matches_read.restype = C.c_int
    L.fs_matches_read.argtypes = [C.c_void_p, u32p, u32p, u32p, C.POINTER(C.c_double),
                                  C.POINTER(C.c_double), C.c_void_p, C.c_uint64, C.c_void_p,
                                  C.c_uint64]
    L.fs_matches_labels.restype = C.c_int
    L.fs_matches_labels.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, u32p, u64p]
    L.fs_variants.restype = C.c_int
    L.fs_variants.argtypes = [C.c_int, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                              C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.fs_readings.restype = C.c_int
    L.fs_readings.argtypes = [C.c_int, u32p, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                              C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                              C.c_void_p, C.c_uint64, u64p, u64p, u64p]
    L.fs_fanon.restype = C.c_int
    L.fs_fanon.argtypes = [C.c_int, u32p, u64p, C.c_uint32, C.c_uint32, u32p, u64p, C.c_uint32,
                           C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                           C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p, u64p, u64p, u64p,
                           u64p]
    L.fs_fanon_dev.restype = C.c_int
    L.fs_fanon_dev.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                               C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                               C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                               C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p,
                               u64p, u64p, u64p, u64p]
    L.fs_retellings.restype = C.c_int
    L.fs_retellings.argtypes = [C.c_int, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                                C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.fs_retellings_rows.restype = C.c_int
    L.fs_retellings_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                     C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.fs_alignments.restype = C.c_int
    L.fs_alignments.argtypes = [C.c_int, u32p, u32p, u32p, C.POINTER(C.c_double), C.c_uint64,
                                C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                C.c_uint64, u64p, C.c_void_p, C.c_uint64, u64p]
    L.fs_alignments_rows.restype = C.c_int
    L.fs_alignments_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                     C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, u64p,
                                     C.c_void_p, C.c_uint64, u64p]
    L.fs_matrix.restype = C.c_int
    L.fs_matrix.argtypes = [C.c_int, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                            C.c_uint32, u32p, C.c_void_p, C.c_uint64, u64p, u64p]
    L.fs_matrix_rows.restype = C.c_int
    L.fs_matrix_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                 C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, u64p, u64p]
    L.fs_matches_intern.restype = C.c_int
    L.fs_matches_intern.argtypes = [C.c_void_p, C.c_uint32, u32p, u32p, C.c_uint64, u64p]
    L.fs_matches_intern_times.restype = C.c_int
    L.fs_matches_intern_times.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.fs_matches_close.restype = None
    L.fs_matches_close.argtypes = [C.c_void_p]
    L.fs_matches_parse_double.restype = C.c_int
    L.fs_matches_parse_double.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_double)]
    L.fs_search_corpus_begin.restype = C.c_int
    L.fs_search_corpus_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int,
                                         C.POINTER(C.c_uint32)]
    L.fs_search_corpus_end.restype = C.c_int
    L.fs_search_corpus_end.argtypes = [C.c_void_p, C.c_uint32, u64p, C.POINTER(abi.FsStats)]
    L.fs_index_set_scan_timing.restype = C.c_int
    L.fs_index_set_scan_timing.argtypes = [C.c_void_p, C.c_uint32]
    L.fs_search_kernel_name.restype = C.c_char_p
    L.fs_search_kernel_name.argtypes = [C.c_void_p, C.c_void_p]
    L.fs_index_reload_switches.restype = C.c_int
    L.fs_index_reload_switches.argtypes = [C.c_void_p]
    for name in TIMED:                 # (the stage times of the command's last call)
        fn = getattr(L, "fs_%s_times" % name)
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_double)]
    optional = {                       # (absent from older builds loaded through FS_LIB_FILE)
        "fs_debug_stamps": [C.c_void_p, C.c_uint32, u64p, C.c_uint64, u64p],
        "fs_debug_ids16_window": [C.POINTER(C.c_uint16), C.c_uint64, C.c_uint32, u32p],
        "fs_stream_floor": [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_double)],
        "fs_index_scan_shape": [C.c_void_p, C.c_void_p, C.POINTER(abi.FsScanShape)],
        "fs_index_share_counts": [C.c_void_p, u64p],
        "fs_index_lsh_counts": [C.c_void_p, u64p],
        "fs_index_share_info": [C.c_void_p, u32p, u32p, u32p, C.POINTER(C.c_double)],
        "fs_index_component_sizes": [C.c_void_p, u32p, C.c_uint64, u64p, u32p],
        "fs_search_profile": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int,
                              C.c_char_p, C.c_uint64, C.POINTER(C.c_double), C.c_uint32,
                              C.POINTER(C.c_uint32)]}
    for name, argtypes in optional.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = C.c_int, argtypes
    L.fs_scan_benchmark.restype = C.c_int
    L.fs_scan_benchmark.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32,
                                    C.POINTER(C.c_double)]
    if L.fs_version() != 1:
        raise RuntimeError("ABI version mismatch in %s" % path)
    _LIB = L
    return L


def check(rc, where):
    if rc != abi.FS_OK:
        L = load()
        detail = L.fs_strerror(rc).decode()
        last = L.fs_last_error().decode()
        if last:
            detail += ": " + last
        raise FsError(rc, where, detail)
