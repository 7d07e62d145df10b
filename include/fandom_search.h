/* fandom_search.h -- C ABI of the MI355X 6-gram text-reuse search library
 * (libfandomsearch_hip.so).
 *
 * The reference (senderle/fandom-search) is pure Python and has no FFI; its
 * seams for this path are Python call sites.  Each entry point below names the
 * reference interface it stands behind (file:line in the reference tree):
 *
 *   fs_index_create      AnnIndexSearch.__init__ + build_lsh_engine
 *                        (search.py:131-154, 86-124): script tokens -> LSH index
 *   fs_corpus_create     the per-work read + tokenise + mk_vectors step of
 *                        AnnIndexSearch.search (search.py:164-173), batched:
 *                        packed vector-id / string-id buffers for many works
 *   fs_search_corpus     AnnIndexSearch.search (search.py:163-226) over every
 *                        work of a corpus, i.e. one pool.map batch
 *                        (search.py:381-386) in a single call
 *   fs_search            convenience: fs_corpus_create + fs_search_corpus +
 *                        fs_corpus_destroy on host buffers
 *   fs_stats             AnnIndexSearch.windows_processed / reset_stats
 *                        (search.py:156-161) plus kernel timings
 *
 * Conventions: every function returns FS_OK (0) or a negative FS_E_* code and
 * never throws across the boundary; the caller owns every buffer it passes,
 * the library owns only the opaque handles; a handle is bound to one device
 * and is not thread-safe (use one handle per device / per rank).  Rows come
 * back sorted by (work, fan_ix) -- the order of `sorted(values)` at
 * search.py:226 followed by the in-order concatenation of search.py:386.
 *
 * Data model
 *   vector id   uint32.  id < n_vec: row of the embedding matrix `emb`.
 *               id & FS_OOV_FLAG: out-of-vocabulary 3-hot vector of
 *               search.py:79-83, low 31 bits = (a*D + b)*D + c, a <= b <= c.
 *               Two tokens have equal vector ids iff they have equal vectors.
 *   string      UTF-32 code points in a string table: chars[off[i]..off[i+1])
 *   work        tokens [work_off[w], work_off[w+1]) of the packed buffers
 */
#ifndef FANDOM_SEARCH_H
#define FANDOM_SEARCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FS_ABI_VERSION 1
#define FS_OOV_FLAG 0x80000000u

enum {
  FS_OK = 0,
  FS_E_INVALID = -1,      /* bad argument / inconsistent sizes                */
  FS_E_NOMEM = -2,        /* host or device allocation failed                 */
  FS_E_DEVICE = -3,       /* HIP runtime error (fs_last_error has the text)   */
  FS_E_CAPACITY = -4,     /* rows buffer too small; *n_rows = rows required   */
  FS_E_UNSUPPORTED = -5,  /* parameter outside what the kernels are built for */
  FS_E_UNPROVEN = -6      /* mode FS_MODE_EXACT but the prefilter proof fails */
};

/* which device pipeline produced (or will produce) the rows */
enum {
  FS_MODE_AUTO = 0,     /* exact n-gram scan when the index proves it sound,
                           otherwise the general LSH pipeline                 */
  FS_MODE_GENERAL = 1,  /* always the LSH pipeline (A6/A12 of SURVEY 8(a))    */
  FS_MODE_EXACT = 2     /* exact scan or FS_E_UNPROVEN                        */
};

typedef struct fs_config {
  uint32_t struct_size;        /* sizeof(fs_config), for ABI growth           */
  uint32_t window_size;        /* n            search.py:337  default 6       */
  uint32_t number_of_hashes;   /* H            search.py:338  default 15      */
  uint32_t hash_dimensions;    /* B <= 24      search.py:339  default 14      */
  uint32_t emb_dim;            /* D            300 for en_core_web_md         */
  uint32_t nearest_n;          /* NearPy NearestFilter(N) default 10          */
  uint32_t unique_filter;      /* NearPy UniqueFilter on fetch: 0 = NearPy 1.0.0 for the reference's call (host default), 1 = NearPy 0.2.x */
  uint32_t mode;               /* FS_MODE_*                                   */
  int32_t  device;             /* HIP device ordinal                          */
  uint32_t reserved;
  double   distance_threshold; /*              search.py:340  default 0.1     */
} fs_config;

/* One output record = the numeric half of a row of new_record_structure
 * (search.py:20-37); the host joins file name, words, orth ids, character and
 * scene by (work, fan_ix, orig_ix). */
typedef struct fs_row {
  uint32_t work;     /* index into work_off                                   */
  uint32_t fan_ix;   /* FAN_WORK_WORD_INDEX                                   */
  uint32_t orig_ix;  /* ORIGINAL_SCRIPT_WORD_INDEX                            */
  uint32_t lev;      /* BEST_LEVENSHTEIN_DISTANCE                             */
  double   dist;     /* BEST_MATCH_DISTANCE                                   */
  double   comb;     /* BEST_COMBINED_DISTANCE = dist * lev                   */
} fs_row;            /* 32 bytes                                              */

typedef struct fs_stats {
  uint64_t windows_processed;  /* search.py:177 counter, summed over works     */
  uint64_t candidates;         /* scan: filter positives; LSH: bucket entries */
  uint64_t matches;            /* (window, script window) pairs kept          */
  uint64_t rows;               /* records after per-word dedupe               */
  double   scan_ms;            /* dominant kernel, HIP-event time; 0 if untimed */
  double   total_ms;           /* all device work of the call, HIP events; fs_search_corpus
                                  and fs_search only (0 for _begin/_end pairs and on
                                  searches without timing, fs_index_set_scan_timing) */
  uint32_t path;               /* FS_MODE_GENERAL or FS_MODE_EXACT            */
  uint32_t scan_launches;      /* launches of the dominant kernel in the call */
  uint32_t lsh_pending;        /* general pipeline: candidate windows that took the full LSH
                                  path (keys, buckets, distances), a wave each; the others
                                  ended in the lane-per-candidate steps                  */
  uint32_t handoff_fallbacks;  /* times this call ran its search again through the chained
                                  kernels because the in-launch hand-off of k_scan_rows gave
                                  up (a workgroup waited longer than a few scan times for
                                  the ones in front: co-residency lost); 0 in normal running */
} fs_stats;

typedef struct fs_index_info {
  uint32_t path;            /* pipeline fs_search_corpus will run             */
  uint32_t proof_ok;        /* exact-n-gram prefilter proven sound            */
  double   c_max;           /* max cosine between distinct vectors            */
  double   cos_bound;       /* upper bound on cos(F,S) with >= 1 mismatch     */
  double   norm_min, norm_max;
  uint64_t n_script;        /* script tokens                                  */
  uint64_t n_windows;       /* script windows                                 */
  uint64_t n_grams;         /* distinct script n-grams (by vector id)         */
  uint64_t filter_bytes;    /* size of the LDS-resident n-gram filter         */
} fs_index_info;

typedef struct fs_index fs_index;
typedef struct fs_corpus fs_corpus;

int fs_version(void);
const char* fs_strerror(int code);
/* text of the last FS_E_DEVICE / FS_E_INVALID on this thread */
const char* fs_last_error(void);

/* Build the script index on cfg->device.
 *   script_vec[n_script]        vector id of each (lower-cased) script word
 *   script_chars/script_off     text of each script word: word i is
 *                               script_chars[script_off[i]..script_off[i+1])
 *   emb[n_vec][D] float32       vector table (spaCy vectors.data)
 *   normals[H][B][D*n] float64  LSH hyperplanes (NearPy draws them unseeded,
 *                               search.py:114-115; here they are an input)   */
int fs_index_create(const fs_config* cfg,
                    const uint32_t* script_vec,
                    const uint32_t* script_chars, const uint64_t* script_off,
                    uint64_t n_script,
                    const float* emb, uint64_t n_vec,
                    const double* normals,
                    fs_index** out);
int fs_index_info_get(const fs_index* ix, fs_index_info* info);
void fs_index_destroy(fs_index* ix);

/* Upload a batch of works (host buffers) to the index's device.
 *   tok_vec[n_tok]   vector id per fan token (what the kernels scan)
 *   tok_str[n_tok]   string id per fan token, or NULL when string id ==
 *                    vector id (synthetic corpora)
 *   str_chars/str_off/n_str   string table of the fan side
 *   work_off[n_works+1]       token offsets, work_off[0] == 0               */
int fs_corpus_create(fs_index* ix,
                     const uint32_t* tok_vec, const uint32_t* tok_str,
                     const uint64_t* work_off, uint64_t n_works,
                     const uint32_t* str_chars, const uint64_t* str_off,
                     uint64_t n_str,
                     fs_corpus** out);
/* A corpus may be destroyed before or after its index: fs_index_destroy detaches
 * the corpora that are still alive (a detached corpus can only be destroyed). */
void fs_corpus_destroy(fs_corpus* c);

/* A corpus of `ix` that searches the works of `base` (a corpus of another index on the same
 * device, with the same window size, emb_dim and vector count) without copying them: the token,
 * string-id, work-offset and block tables are base's, every per-index table is the view's own.
 * One batch searched with several scripts is uploaded once (`ao3.py search` with several
 * scripts).  A view reads the base's buffers and sizes at every search, so it follows
 * fs_corpus_update_begin/_end on the base, and rebuilds its own tables at its first search after
 * one, on its own index's stream, behind the base's upload (a device-side wait on the base's
 * copy).  The base cannot be updated while a search of one of its views is in flight.
 * fs_corpus_update_begin/_end on a view are refused.  A view may be destroyed at any time;
 * destroying the base detaches its views (a detached view can only be destroyed).
 * FS_E_INVALID for a base of `ix` itself, a view as base, another device, or a different
 * window size, emb_dim or vector count (fs_last_error says which). */
int fs_corpus_view(fs_index* ix, fs_corpus* base, fs_corpus** out);

/* Streaming (BASELINE configs[4]: corpora larger than one batch, streamed from
 * pinned host memory).  fs_corpus_update_begin replaces the works of `c` with a
 * new batch: the copies, the block->work table and a device-side validation of
 * the ids are queued on the corpus's own copy stream and the call returns at
 * once, so the upload overlaps a search that is running on another corpus of
 * the same index.  The host buffers must stay untouched until
 * fs_corpus_update_end (or the next fs_search_corpus on `c`) has returned.
 * The string table given at fs_corpus_create is kept.  Use fs_host_alloc for
 * the staging buffers: copies from pageable memory do not overlap. */
int fs_corpus_update_begin(fs_corpus* c, const uint32_t* tok_vec, const uint32_t* tok_str,
                           const uint64_t* work_off, uint64_t n_works);
int fs_corpus_update_end(fs_corpus* c);
int fs_host_alloc(uint64_t bytes, void** out);
void fs_host_free(void* p);

/* where fs_search_corpus leaves the records */
enum {
  FS_ROWS_HOST = 0,           /* `rows` is a host buffer of fs_row                        */
  FS_ROWS_DEVICE = 1,         /* `rows` is a device buffer of fs_row                      */
  FS_ROWS_DEVICE_PACKED = 2,  /* `rows` is a device buffer of 16-byte wire records
                                 {work, fan_ix, orig_ix, lev | k << 16} (exact n-gram
                                 pipeline only, else FS_E_UNSUPPORTED): half the bytes
                                 for the gather; fs_rows_unpack restores fs_row          */
  FS_ROWS_DEVICE_PACKED8 = 3, /* 8-byte wire records {token position in the batch,
                                 orig_ix | k << 18 | lev << 22}: a quarter of the bytes.
                                 Exact pipeline and scripts below 2^18 tokens only
                                 (else FS_E_UNSUPPORTED); fs_rows_unpack8 restores fs_row
                                 given the batch's work offsets                          */
  FS_ROWS_HEADER = 0x100      /* flag, with a device mode: `rows` points to a 32-byte
                                 header followed by the `cap` records; the search writes
                                 the record count (uint64) into the header's first eight
                                 bytes, so that count and records can travel in one
                                 collective without a host-side step in between          */
};

/* Search every work of `c`.  `rows` is a host buffer of `cap` records, or,
 * when rows_on_device != 0, a 16-byte aligned device pointer on the index's
 * device (for a collective gather without a host round trip).  On FS_E_CAPACITY *n_rows is
 * the number required.  `st` may be NULL. */
int fs_search_corpus(fs_index* ix, fs_corpus* c,
                     fs_row* rows, uint64_t cap, int rows_on_device,
                     uint64_t* n_rows, fs_stats* st);

/* The same in two halves: _begin queues the search and returns a ticket, _end waits
 * for it and delivers what fs_search_corpus delivers.  Up to four searches may be in
 * flight per index, so the host can queue the next batch while the GPU still works
 * on the previous ones.  With FS_LANES=2..4 in the environment consecutive searches
 * go to alternating streams of the index and overlap on the GPU (the verify / rows
 * chain of one beside the scan of the next; searches are independent, every one
 * writes only its own rows buffer); by default they run in order.  Device row modes
 * only while another search is in flight; the rows buffers of searches in flight
 * must be distinct; a corpus must not be updated while a search on it is in
 * flight. */
int fs_search_corpus_begin(fs_index* ix, fs_corpus* c, fs_row* rows, uint64_t cap,
                           int rows_mode, uint32_t* ticket);
int fs_search_corpus_end(fs_index* ix, uint32_t ticket, uint64_t* n_rows, fs_stats* st);

/* Expand n packed wire records (device) into fs_row records (device) on an index
 * built from the same script, vectors and config: dist = the matched script
 * window's self distance, comb = dist * lev. */
int fs_rows_unpack(fs_index* ix, const void* packed, uint64_t n, fs_row* rows);

/* The same for n 8-byte wire records: work_off (device, n_works + 1 offsets of the
 * batch the records come from) turns a token position back into (work, fan_ix). */
int fs_rows_unpack8(fs_index* ix, const void* packed, uint64_t n, const uint64_t* work_off,
                    uint64_t n_works, fs_row* rows);

/* fs_corpus_create + fs_search_corpus + fs_corpus_destroy. */
int fs_search(fs_index* ix,
              const uint32_t* tok_vec, const uint32_t* tok_str,
              const uint64_t* work_off, uint64_t n_works,
              const uint32_t* str_chars, const uint64_t* str_off,
              uint64_t n_str,
              fs_row* rows, uint64_t cap, uint64_t* n_rows, fs_stats* st);

/* `ao3.py format` aggregation (ao3.py:351-363, 407-416): for every script word the
 * number of match records whose BEST_COMBINED_DISTANCE is <= each of `n_thr`
 * ascending thresholds (the reference uses 0, 0.05, ... 0.5), plus, in column
 * n_thr, the number of records of that word at all.
 *   orig_ix[n_rows], comb[n_rows]   host arrays (two columns of the match CSV)
 *   counts[n_script][n_thr + 1]     host, uint32
 * NaN never satisfies <=, as in pandas.  Runs on HIP device `device`. */
int fs_reuse_histogram(int device, const uint32_t* orig_ix, const double* comb, uint64_t n_rows,
                       uint64_t n_script, const double* thresholds, uint32_t n_thr,
                       uint32_t* counts);
/* The same over device-resident fs_row records (e.g. straight after a search or a
 * gather); d_counts is a device buffer of n_script * (n_thr + 1) uint32. */
int fs_reuse_histogram_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                            const double* thresholds, uint32_t n_thr, uint32_t* d_counts);

/* `ao3.py passages`: match records joined into passages of reuse.  Records are sorted by
 * (work, fan_ix) (what fs_search_corpus returns); record s continues the run of the record r
 * just before it when s.work == r.work, 1 <= s.fan_ix - r.fan_ix <= 1 + max_gap and
 * 1 <= s.orig_ix - r.orig_ix <= 1 + max_gap (signed differences; a repeated fan_ix ends a run).
 * Runs of at least min_words records are passages, in record order.  Sums start at +0.0 and
 * add the records in order; maxima are over non-NaN values, the earlier record kept on a tie
 * (NaN only when every value is NaN); n_exact counts comb <= 0 (NaN never). */
typedef struct fs_passage {
  uint64_t first;      /* index of the passage's first record                  */
  uint32_t n_words;    /* records in the passage                               */
  uint32_t n_exact;    /* records with comb <= 0                               */
  double   dist_sum, dist_max;
  double   comb_sum, comb_max;
} fs_passage;          /* 48 bytes                                             */

/* Host columns in, `cap` host passages out, on HIP device `device`.  Here and in every
 * command below, the host form uploads its columns, packs them on the device into fs_row
 * records (lev 0; a column the command does not take 0.0) and runs what its _rows form runs:
 * it holds 32 bytes per record on the device, and the columns beside them only while it
 * packs.  Both entry points:
 * FS_E_INVALID for min_words == 0 or records out of (work, fan_ix) order, FS_E_UNSUPPORTED
 * for n_rows >= 2^32, FS_E_CAPACITY with *n_out = passages required when cap is smaller,
 * FS_OK with *n_out = 0 and no device work for n_rows == 0. */
int fs_passages(int device, const uint32_t* work, const uint32_t* fan_ix, const uint32_t* orig_ix,
                const double* dist, const double* comb, uint64_t n_rows, uint32_t min_words,
                uint32_t max_gap, fs_passage* out, uint64_t cap, uint64_t* n_out);
/* The same over fs_row records already on the device (16-byte aligned, e.g. straight after a
 * search; lev is not read) into a device buffer of `cap` passages, on the index's device and
 * stream; returns when they are written. */
int fs_passages_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t min_words,
                     uint32_t max_gap, fs_passage* d_out, uint64_t cap, uint64_t* n_out);

/* `ao3.py works`: the same records reduced by work.  Records are sorted by (work, fan_ix) as
 * for fs_passages; group_of[n_script] (host memory in both entry points, or NULL with
 * n_groups = 0) maps a script word to a group id < n_groups, e.g. its scene or its character.
 * Every output is an integer, so the result does not depend on the order in which the
 * kernels combine records.  A work without records gets zeros and top_group = 0xFFFFFFFF. */
typedef struct fs_work {
  uint64_t first;            /* index of the work's first record                        */
  uint32_t n_words;          /* its records                                             */
  uint32_t fan_first;        /* fan_ix of its first ...                                 */
  uint32_t fan_last;         /* ... and last record (the smallest and largest)          */
  uint32_t n_script_words;   /* distinct orig_ix among its records                      */
  uint32_t n_passages;       /* passages under (min_words, max_gap) as fs_passages      */
  uint32_t passage_words;    /* records inside them                                     */
  uint32_t longest;          /* records in the longest                                  */
  uint32_t n_groups_hit;     /* distinct groups among its records (= its cells)         */
  uint32_t top_group;        /* group with the most records, the smallest id on a tie   */
  uint32_t top_group_words;  /* records of that group                                   */
  uint32_t reserved, reserved2;   /* 0                                                  */
} fs_work;                   /* 56 bytes                                                */

/* one (work, group) pair that has a record; the list is sorted by (work, group) */
typedef struct fs_work_cell {
  uint32_t work, group;
  uint32_t n_words;          /* records of the pair                                     */
  uint32_t n_exact;          /* ... with comb <= 0 (NaN never)                          */
} fs_work_cell;              /* 16 bytes                                                */

#define FS_WORKS_MAX_SCRIPT (1u << 19)   /* n_script and n_groups up to these; beyond them     */
#define FS_WORKS_MAX_GROUPS 4096u        /* both entry points return FS_E_UNSUPPORTED          */

/* Host columns in; out[n_works], counts[n_works][n_thr + 1] (records with comb <= each of the
 * n_thr ascending thresholds, NaN never, as fs_reuse_histogram; column n_thr = all records of
 * the work) and `cap` cells out, on HIP device `device`.  Both entry points: FS_E_INVALID for
 * min_words == 0, n_thr outside 1..64, thresholds that do not ascend, records out of
 * (work, fan_ix) order, a work >= n_works, an orig_ix >= n_script or a group_of entry >=
 * n_groups; FS_E_UNSUPPORTED for n_rows >= 2^32, n_script > FS_WORKS_MAX_SCRIPT or n_groups >
 * FS_WORKS_MAX_GROUPS; FS_E_CAPACITY with *n_cells = cells required when cap is smaller (out
 * and counts are complete then).  n_rows == 0: empty summaries, zero counts, *n_cells = 0
 * (fs_works: without device work). */
int fs_works(int device, const uint32_t* work, const uint32_t* fan_ix, const uint32_t* orig_ix,
             const double* comb, uint64_t n_rows, uint32_t n_works, uint32_t n_script,
             const uint32_t* group_of, uint32_t n_groups, uint32_t min_words, uint32_t max_gap,
             const double* thresholds, uint32_t n_thr, fs_work* out, uint32_t* counts,
             fs_work_cell* cells, uint64_t cap, uint64_t* n_cells);
/* The same over device-resident fs_row records (16-byte aligned) into device buffers (d_out
 * 8-byte, d_cells 16-byte aligned), n_script taken from the index, on the index's device and
 * stream; returns when they are written. */
int fs_works_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                  const uint32_t* group_of, uint32_t n_groups, uint32_t min_words,
                  uint32_t max_gap, const double* thresholds, uint32_t n_thr, fs_work* d_out,
                  uint32_t* d_counts, fs_work_cell* d_cells, uint64_t cap, uint64_t* n_cells);

/* `ao3.py quotes`: the same records seen from the script's side.  Records are sorted by
 * (work, fan_ix) as for fs_passages, and a passage is what fs_passages keeps under
 * (min_words, max_gap).  Its span is [orig_ix of its first record, orig_ix of its last]; it
 * covers every script word in the span, the words it bridges under max_gap too.  Every output
 * is an integer, so the result does not depend on the order in which the kernels combine
 * records or passages. */
typedef struct fs_quote_word {
  uint32_t n_words;          /* records with orig_ix == this word, in a passage or not  */
  uint32_t n_exact;          /* ... with comb <= 0 (NaN never)                          */
  uint32_t n_works;          /* distinct works with a record at the word                */
  uint32_t n_passages;       /* passages covering the word                              */
  uint32_t n_passage_works;  /* distinct works with a passage covering it: its depth    */
  uint32_t region;           /* index of the region holding the word, or 0xFFFFFFFF     */
} fs_quote_word;             /* 24 bytes                                                */

/* A region: a maximal run of consecutive script words of depth >= min_works; regions are
 * numbered in script order.  Its first and last word always carry a record. */
typedef struct fs_quote_region {
  uint32_t first, last;      /* script word indices, inclusive                          */
  uint32_t n_passages;       /* passages whose span intersects [first, last]            */
  uint32_t n_works;          /* distinct works with such a passage                      */
  uint32_t n_words, n_exact; /* sums of the words' n_words and n_exact                  */
  uint32_t peak;             /* largest depth in the region                             */
  uint32_t peak_first;       /* smallest word index at the peak                         */
  uint32_t peak_last;        /* end of the run of words at the peak that starts there   */
  uint32_t reserved;         /* 0                                                       */
} fs_quote_region;           /* 40 bytes                                                */

/* Host columns in; words[n_script] and `cap` regions out, on HIP device `device`.  Both entry
 * points: FS_E_INVALID for min_words == 0, min_works == 0, records out of (work, fan_ix)
 * order, a work >= n_works or an orig_ix >= n_script; FS_E_UNSUPPORTED for n_rows >= 2^32 or
 * n_script > FS_WORKS_MAX_SCRIPT; FS_E_CAPACITY with *n_regions = regions required when cap is
 * smaller (words is complete then).  n_rows == 0: zeroed words with region = 0xFFFFFFFF,
 * *n_regions = 0 (fs_quotes: without device work). */
int fs_quotes(int device, const uint32_t* work, const uint32_t* fan_ix, const uint32_t* orig_ix,
              const double* comb, uint64_t n_rows, uint32_t n_works, uint32_t n_script,
              uint32_t min_words, uint32_t max_gap, uint32_t min_works, fs_quote_word* words,
              fs_quote_region* regions, uint64_t cap, uint64_t* n_regions);
/* The same over device-resident fs_row records (16-byte aligned) into device buffers (4-byte
 * aligned), n_script taken from the index, on the index's device and stream; returns when
 * they are written. */
int fs_quotes_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                   uint32_t min_words, uint32_t max_gap, uint32_t min_works,
                   fs_quote_word* d_words, fs_quote_region* d_regions, uint64_t cap,
                   uint64_t* n_regions);

/* `ao3.py pairs`: fan works related by the script words both quote.  Records and passages as
 * for fs_quotes.  The coverage C_w of work w is the union, over its passages, of every script
 * word from the passage's first record to its last (bridged words too); a work without a
 * passage has none.  For works a < b, shared = |C_a & C_b|; the pair is kept when shared >=
 * min_shared.  Every output is an integer. */
typedef struct fs_pair_work {
  uint32_t covered;          /* |C_w|; 0 for a work without a passage                   */
  uint32_t partners;         /* kept pairs the work is in                               */
  uint32_t best;             /* the partner with the largest shared, the smaller work
                                number on a tie; 0xFFFFFFFF without partners            */
  uint32_t best_shared;      /* its shared; 0 without partners                          */
} fs_pair_work;              /* 16 bytes                                                */

typedef struct fs_pair {
  uint32_t a, b;             /* work numbers, a < b                                     */
  uint32_t shared;           /* script words in both coverages                          */
  uint32_t first, last;      /* smallest and largest of them                            */
  uint32_t run_first;        /* start of the longest run of consecutive script words in
                                both coverages, the first one among equals              */
  uint32_t run_words;        /* its length                                              */
  uint32_t reserved;         /* 0                                                       */
} fs_pair;                   /* 32 bytes                                                */

/* The coverage matrix is a row of ceil(n_script / 64) 64-bit words per active work (a work
 * with a passage): active_works * ceil(n_script / 64) * 8 bytes may be up to this. */
#define FS_PAIRS_MAX_BYTES (1u << 30)

/* Host columns in; works[n_works] and `cap` pairs out, on HIP device `device`.  The pairs come
 * in (a, b) ascending order.  Both entry points: FS_E_INVALID for min_words == 0, min_shared ==
 * 0, records out of (work, fan_ix) order, a work >= n_works or an orig_ix >= n_script;
 * FS_E_UNSUPPORTED for n_rows >= 2^32, n_script > FS_WORKS_MAX_SCRIPT or a coverage matrix
 * above FS_PAIRS_MAX_BYTES; FS_E_CAPACITY with *n_pairs = pairs required when cap is smaller
 * (works is complete then, pairs untouched).  n_rows == 0: works without coverage, *n_pairs = 0
 * (fs_pairs: without device work). */
int fs_pairs(int device, const uint32_t* work, const uint32_t* fan_ix, const uint32_t* orig_ix,
             uint64_t n_rows, uint32_t n_works, uint32_t n_script, uint32_t min_words,
             uint32_t max_gap, uint32_t min_shared, fs_pair_work* works, fs_pair* pairs,
             uint64_t cap, uint64_t* n_pairs);
/* The same over device-resident fs_row records (16-byte aligned) into device buffers (16-byte
 * aligned), n_script taken from the index, on the index's device and stream; returns when
 * they are written. */
int fs_pairs_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                  uint32_t min_words, uint32_t max_gap, uint32_t min_shared,
                  fs_pair_work* d_works, fs_pair* d_pairs, uint64_t cap, uint64_t* n_pairs);
/* HIP-event milliseconds of the last fs_pairs / fs_pairs_rows call on this thread: coverage
 * matrix, count pass (with its scan), place pass, detail pass; 0 for a pass that did not run.
 * tools/pairs_bench.py. */
int fs_pairs_times(double* ms);

/* `ao3.py clusters`: families of fan works quoting the same lines.  Records, passages and
 * coverage as for fs_pairs; a work with a passage is active.  Active works a < b are linked when
 * shared = |C_a & C_b| >= min_shared and 100 * shared >= min_jaccard * (|C_a| + |C_b| - shared)
 * (min_jaccard: a whole percentage, 0..100; equality links; at 0 the rule is that of fs_pairs).
 * A family is a connected component of the links over the active works, so two works that
 * share nothing may be in one family through a third; a single active work is a family of one.
 * A family of at least min_size works is listed.  The depth of script word o in a family is the
 * number of its members whose coverage holds o.  Every output is an integer. */
typedef struct fs_cluster_work {
  uint32_t covered;          /* |C_w|; 0 for a work without a passage                   */
  uint32_t root;             /* smallest work number of its family; 0xFFFFFFFF for a
                                work without a passage                                  */
  uint32_t size;             /* works in its family; 0 for a work without a passage     */
  uint32_t cluster;          /* index of its family among the listed ones; 0xFFFFFFFF
                                when the family is not listed                           */
  uint32_t links;            /* links the work is in                                    */
  uint32_t best;             /* the linked partner with the largest shared, the smaller
                                work number on a tie; 0xFFFFFFFF without links          */
  uint32_t best_shared;      /* its shared; 0 without links                             */
  uint32_t reserved;         /* 0                                                       */
} fs_cluster_work;           /* 32 bytes                                                */

typedef struct fs_cluster {
  uint32_t root;             /* smallest work number of the family                      */
  uint32_t n_works;          /* its works                                               */
  uint32_t n_links;          /* links inside it (0xFFFFFFFF: that many or more)         */
  uint32_t hub;              /* the member with the most links, the smaller work number
                                on a tie                                                */
  uint32_t hub_links;        /* its links                                               */
  uint32_t covered;          /* script words of depth >= 1                              */
  uint32_t common;           /* script words of depth >= t,
                                t = (common_pct * n_works + 99) / 100                   */
  uint32_t peak;             /* the largest depth                                       */
  uint32_t peak_first;       /* smallest word index at the peak                         */
  uint32_t run_first;        /* start of the longest run of consecutive script words of
                                depth >= t, the first one among equals; 0xFFFFFFFF when
                                common == 0                                             */
  uint32_t run_words;        /* its length; 0 when common == 0                          */
  uint32_t reserved;         /* 0                                                       */
} fs_cluster;                /* 48 bytes                                                */

/* Counted against this, with A = the active works, nk = ceil(n_script / 64) and before the
 * work x work product runs:
 *   the coverage rows              A * nk * 8
 *   the rows of common-word masks  (A / min_size) * nk * 8, one per listed family at the
 *                                  most families of min_size works there can be
 * The per-work and per-family tables of a few words each, the records, the run heads and the
 * outputs are not counted. */
#define FS_CLUSTERS_MAX_BYTES (1u << 30)

/* Host columns in; works[n_works] and `cap` listed families out, on HIP device `device`.  The
 * families come in ascending order of root.  Both entry points: FS_E_INVALID for min_words,
 * min_shared, min_size or common_pct == 0, min_jaccard > 100, common_pct > 100, records out of
 * (work, fan_ix) order, a work >= n_works or an orig_ix >= n_script; FS_E_UNSUPPORTED for
 * n_rows >= 2^32, n_script > FS_WORKS_MAX_SCRIPT or tables above FS_CLUSTERS_MAX_BYTES;
 * FS_E_CAPACITY with *n_clusters = families required when cap is smaller (works is complete
 * then, clusters untouched).  n_rows == 0: works without coverage, *n_clusters = 0
 * (fs_clusters: without device work). */
int fs_clusters(int device, const uint32_t* work, const uint32_t* fan_ix,
                const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works, uint32_t n_script,
                uint32_t min_words, uint32_t max_gap, uint32_t min_shared, uint32_t min_jaccard,
                uint32_t min_size, uint32_t common_pct, fs_cluster_work* works,
                fs_cluster* clusters, uint64_t cap, uint64_t* n_clusters);
/* The same over device-resident fs_row records (16-byte aligned) into device buffers (16-byte
 * aligned), n_script taken from the index, on the index's device and stream; returns when
 * they are written. */
int fs_clusters_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                     uint32_t min_words, uint32_t max_gap, uint32_t min_shared,
                     uint32_t min_jaccard, uint32_t min_size, uint32_t common_pct,
                     fs_cluster_work* d_works, fs_cluster* d_clusters, uint64_t cap,
                     uint64_t* n_clusters);
/* HIP-event milliseconds of the last fs_clusters / fs_clusters_rows call on this thread:
 * coverage matrix, link pass, families (roots, sizes, numbering, member lists, the works),
 * depth pass, merge pass; 0 for a pass that did not run.  tools/clusters_bench.py. */
int fs_clusters_times(double* ms);

/* `ao3.py tree`: how the families of works merge as the bar drops, the single-linkage
 * dendrogram of the active works.  Records, passages and coverage as for fs_pairs; a work with
 * a passage is active, N of them.  Active works a < b have an edge when shared = |C_a & C_b| >=
 * min_shared and level >= min_level, where level is
 *   FS_TREE_JACCARD  shared * 1000000 / (|C_a| + |C_b| - shared), rounded down
 *   FS_TREE_SHARED   shared
 * Edge e comes before edge f when its level is higher, then when its a is smaller, then its b:
 * one strict order over all edges.  The edges are taken in that order and one is kept when its
 * ends are in different families (Kruskal); the kept edges are the merges, at most N - 1, and
 * form the one maximum spanning forest of that order.  Merge k joins the family holding a, its
 * left side, and the family holding b, its right side.  The trees are the connected components
 * of the forest, a lone active work too, ranked by their works, the most first, then by their
 * earliest work.  The leaves are laid out tree by tree in rank order, and inside a tree the
 * left side of its last merge before the right side, recursively.  Every output is an integer;
 * merges, trees and leaves are numbered from 0. */
#define FS_TREE_JACCARD 0u
#define FS_TREE_SHARED 1u

typedef struct fs_tree_merge {
  uint32_t a, b;             /* the edge: work numbers, a < b                           */
  uint32_t level;            /* its level                                               */
  uint32_t shared;           /* script words in both coverages                          */
  uint32_t a_covered;        /* |C_a|                                                   */
  uint32_t b_covered;        /* |C_b|                                                   */
  uint32_t left, right;      /* the merge that made that side; 0xFFFFFFFF when the side
                                is the single work a (left) or b (right)                */
  uint32_t left_works;       /* works of the left side                                  */
  uint32_t right_works;      /* works of the right side                                 */
  uint32_t works;            /* their sum: works of the merged family                   */
  uint32_t first_work;       /* its smallest work number                                */
  uint32_t tree;             /* rank of the tree the merge is in                        */
  uint32_t run_first;        /* start of the longest run of consecutive script words in
                                both coverages, the first one among equals              */
  uint32_t run_words;        /* its length                                              */
  uint32_t reserved;         /* 0                                                       */
} fs_tree_merge;             /* 64 bytes                                                */

typedef struct fs_tree_work {
  uint32_t covered;          /* |C_w|; 0 for a work without a passage, and then the
                                other fields are 0xFFFFFFFF (tree, joined_merge, best,
                                leaf) and 0                                             */
  uint32_t tree;             /* rank of its tree                                        */
  uint32_t tree_works;       /* works in its tree                                       */
  uint32_t edges;            /* merges whose edge ends in the work                      */
  uint32_t joined_merge;     /* the first of them; 0xFFFFFFFF without one               */
  uint32_t joined_level;     /* its level; 0 without one                                */
  uint32_t best;             /* the other end of that edge, which is the work's first
                                edge in the order; 0xFFFFFFFF without one               */
  uint32_t leaf;             /* its place in the leaf order                             */
} fs_tree_work;              /* 32 bytes                                                */

typedef struct fs_tree_level {
  uint32_t level;            /* a level at which merges happen, the highest first       */
  uint32_t merges;           /* merges at exactly this level                            */
  uint32_t merges_above;     /* merges at higher levels                                 */
  uint32_t families;         /* after every merge at this level or above: families of
                                two works or more                                       */
  uint32_t largest;          /* works of the largest of them                            */
  uint32_t joined;           /* active works in one of them                             */
  uint32_t singles;          /* active works in none                                    */
  uint32_t reserved;         /* 0                                                       */
} fs_tree_level;             /* 32 bytes                                                */

/* Counted against this, with A = the active works and nk = ceil(n_script / 64), before the
 * work x work product runs:
 *   the coverage rows        A * nk * 8
 *   the per-work tables      A * FS_TREE_ROW_BYTES: parent and root (4 bytes each), the work's
 *                            best edge of a round (8), the best level and the chosen edge of
 *                            its component (4 and 8), and its slot of the edge list (32)
 * The records, the run heads, the host's copy of the edges and the outputs are not counted. */
#define FS_TREE_MAX_BYTES (1u << 30)
#define FS_TREE_ROW_BYTES 60u
/* Rounds of the forest's construction after which a call gives up (FS_E_DEVICE): every round
 * that finds an edge at least halves the families that still have one, so 2^32 works need 32. */
#define FS_TREE_MAX_ROUNDS 40u

/* Host columns in; works[n_works], `cap_merges` merges in merge order and `cap_levels` levels
 * out, on HIP device `device`.  Both entry points: FS_E_INVALID for min_words == 0, min_shared
 * == 0, a measure that is none of the two, min_level > 1000000 under FS_TREE_JACCARD, records
 * out of (work, fan_ix) order, a work >= n_works or an orig_ix >= n_script; FS_E_UNSUPPORTED
 * for n_rows >= 2^32, n_script > FS_WORKS_MAX_SCRIPT or tables above FS_TREE_MAX_BYTES;
 * FS_E_CAPACITY with *n_merges and *n_levels = the records required when either capacity is
 * smaller (works is complete then, merges and levels untouched).  n_rows == 0: works without
 * coverage, *n_merges = *n_levels = 0 (fs_tree: without device work). */
int fs_tree(int device, const uint32_t* work, const uint32_t* fan_ix, const uint32_t* orig_ix,
            uint64_t n_rows, uint32_t n_works, uint32_t n_script, uint32_t min_words,
            uint32_t max_gap, uint32_t measure, uint32_t min_shared, uint32_t min_level,
            fs_tree_work* works, fs_tree_merge* merges, uint64_t cap_merges,
            uint64_t* n_merges, fs_tree_level* levels, uint64_t cap_levels, uint64_t* n_levels);
/* The same over device-resident fs_row records (16-byte aligned) into device buffers (16-byte
 * aligned), n_script taken from the index, on the index's device and stream; returns when
 * they are written. */
int fs_tree_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                 uint32_t min_words, uint32_t max_gap, uint32_t measure, uint32_t min_shared,
                 uint32_t min_level, fs_tree_work* d_works, fs_tree_merge* d_merges,
                 uint64_t cap_merges, uint64_t* n_merges, fs_tree_level* d_levels,
                 uint64_t cap_levels, uint64_t* n_levels);
/* Of the last fs_tree / fs_tree_rows call on this thread, ms[0 .. 8]: HIP-event milliseconds
 * of the coverage matrix, then summed over the rounds the flatten, best, choose and hook
 * passes, then the detail pass; host milliseconds of the replay and of the whole call; and in
 * ms[8] a count, not a time: the hooking rounds, the rounds that added an edge.  0 for a pass
 * that did not run.  tools/tree_bench.py. */
int fs_tree_times(double* ms);

/* `ao3.py groups`: the same records reduced by groups of works (a year, an author, a tag).
 * Records, passages and coverage as for fs_pairs.  Membership is many-to-many: work w is in the
 * groups mem_grp[mem_off[w] .. mem_off[w + 1]), strictly ascending (a work may be in none, a
 * group may have no work).  The depth of script word o in group g is the number of different
 * member works of g whose coverage holds o.  A label (a scene) is label_of[orig_ix] of a
 * record.  Every output is an integer. */
typedef struct fs_group {
  uint32_t n_works;          /* member works with at least one record                   */
  uint32_t n_passage_works;  /* member works with at least one passage                  */
  uint32_t n_words;          /* records of member works                                 */
  uint32_t n_exact;          /* ... with exact != 0 (fs_groups_rows: comb <= 0)         */
  uint32_t n_passages;       /* passages of member works                                */
  uint32_t passage_words;    /* records inside them                                     */
  uint32_t longest;          /* records in the longest                                  */
  uint32_t covered;          /* script words of depth >= 1                              */
  uint32_t peak;             /* the largest depth                                       */
  uint32_t peak_first;       /* smallest word index at the peak; 0xFFFFFFFF at depth 0  */
  uint32_t top_label;        /* label with the most records, the smallest id on a tie;
                                0xFFFFFFFF without records or with n_labels == 0        */
  uint32_t top_label_words;  /* its records                                             */
  uint32_t n_cells;          /* the group's cells                                       */
  uint32_t n_word_rows;      /* the group's fs_group_word rows (depth >= min_works)     */
  uint32_t reserved, reserved2;   /* 0                                                  */
} fs_group;                  /* 64 bytes                                                */

/* one (group, label) pair that has a record of a member work; sorted by (group, label) */
typedef struct fs_group_cell {
  uint32_t group, label;
  uint32_t n_words;          /* records of the pair                                     */
  uint32_t n_exact;          /* ... exact ones                                          */
  uint32_t n_works;          /* member works with a record at the label                 */
  uint32_t reserved;         /* 0                                                       */
} fs_group_cell;             /* 24 bytes                                                */

/* one (group, script word) pair of depth >= min_works; sorted by (group, word) */
typedef struct fs_group_word {
  uint32_t group, orig_ix;
  uint32_t n_works;          /* the depth                                               */
  uint32_t reserved;         /* 0                                                       */
} fs_group_word;             /* 16 bytes                                                */

/* Counted against this, from the arguments alone and before anything is allocated, with
 * nk = ceil(n_script / 64) and E = mem_off[n_works], the memberships:
 *   the coverage rows            n_works * nk * 8
 *   the depth rows               S * nk * 64 * 4, S = the groups of more than 255 works
 *   records per (work, label)    n_works * n_labels * 8
 *   the (group, label) counters  n_groups * n_labels * 12
 *   rows and cells per block     n_groups * (ceil(nk / 64) + ceil(n_labels / 64)) * 4
 *   the group-major membership   E * 4 + (groups + E / 255 slabs) * 16
 * The records, the run heads and the outputs are not counted. */
#define FS_GROUPS_MAX_BYTES (1u << 30)

/* Host columns and host membership in; groups[n_groups], `cap_cells` cells and `cap_words` word
 * rows out, on HIP device `device`.  label_of[n_script] gives every script word's label <
 * n_labels (NULL with n_labels == 0: no cells, top_label = 0xFFFFFFFF).  Both entry points:
 * FS_E_INVALID for min_words == 0, min_works == 0, records out of (work, fan_ix) order, a work
 * >= n_works, an orig_ix >= n_script, a group >= n_groups, a label >= n_labels, a work's groups
 * not strictly ascending, mem_off not non-decreasing or mem_off[0] != 0; FS_E_UNSUPPORTED for
 * n_rows >= 2^32, n_script > FS_WORKS_MAX_SCRIPT or tables above FS_GROUPS_MAX_BYTES (before
 * anything is allocated); FS_E_CAPACITY with *n_cells and *n_words = the counts required when
 * either buffer is too small (groups is complete then, cells and words untouched).
 * n_rows == 0 or n_groups == 0: groups without counts (peak_first = top_label = 0xFFFFFFFF),
 * *n_cells = *n_words = 0 (fs_groups: without device work). */
int fs_groups(int device, const uint32_t* work, const uint32_t* fan_ix, const uint32_t* orig_ix,
              const uint8_t* exact, uint64_t n_rows, uint32_t n_works, uint32_t n_script,
              const uint64_t* mem_off, const uint32_t* mem_grp, uint32_t n_groups,
              const uint32_t* label_of, uint32_t n_labels, uint32_t min_words, uint32_t max_gap,
              uint32_t min_works, fs_group* groups, fs_group_cell* cells, uint64_t cap_cells,
              uint64_t* n_cells, fs_group_word* words, uint64_t cap_words, uint64_t* n_words);
/* The same over device-resident fs_row records (16-byte aligned; exact: comb <= 0) into device
 * buffers (d_groups and d_words 16-byte, d_cells 8-byte aligned); membership and label_of stay
 * host arrays; n_script taken from the index, on the index's device and stream; returns when
 * they are written. */
int fs_groups_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                   const uint64_t* mem_off, const uint32_t* mem_grp, uint32_t n_groups,
                   const uint32_t* label_of, uint32_t n_labels, uint32_t min_words,
                   uint32_t max_gap, uint32_t min_works, fs_group* d_groups,
                   fs_group_cell* d_cells, uint64_t cap_cells, uint64_t* n_cells,
                   fs_group_word* d_words, uint64_t cap_words, uint64_t* n_words);
/* HIP-event milliseconds of the last fs_groups / fs_groups_rows call on this thread: per-work
 * tables (records, passages, coverage), reduction by group (scalars, labels, depth, counts),
 * offsets, place pass; 0 for a pass that did not run.  tools/groups_bench.py. */
int fs_groups_times(double* ms);

/* `ao3.py variants`: what fans wrote at every script word. A record is (work, orig_ix, spell),
 * spell the id of its fan word's spelling (fs_matches_intern, or any dense numbering); records
 * come in any order, every output is a count or a distinct count.  A cell is a (script word,
 * spelling) pair that has a record. */
typedef struct fs_variant_cell {
  uint32_t orig_ix, spell;
  uint32_t n_records;        /* records of the pair                                     */
  uint32_t n_works;          /* distinct works among them                               */
} fs_variant_cell;           /* 16 bytes                                                */

typedef struct fs_variant_word {
  uint32_t n_records;        /* records with orig_ix == this word                       */
  uint32_t n_spellings;      /* distinct spellings among them (= its cells)             */
  uint32_t n_works;          /* distinct works among them                               */
  uint32_t first_cell;       /* index of its first cell, its top spelling; 0xFFFFFFFF for
                                a word without records                                  */
} fs_variant_word;           /* 16 bytes                                                */

/* Host columns in; words[n_script] and `cap` cells out, on HIP device `device`.  The cells are
 * sorted by orig_ix ascending, then n_records descending, then n_works descending, then spell
 * ascending: a total order, so the output does not depend on the order of the records.
 * FS_E_INVALID for a work >= n_works, an orig_ix >= n_script or a spell >= n_spell;
 * FS_E_UNSUPPORTED for n >= 2^32 or n_script > FS_WORKS_MAX_SCRIPT; FS_E_CAPACITY with *n_cells
 * = cells required when cap is smaller (words is complete then).  n == 0: zeroed words with
 * first_cell = 0xFFFFFFFF, *n_cells = 0, without device work.  There is no _rows twin: fs_row
 * carries no fan word, so records a search left on the device cannot feed this. */
int fs_variants(int device, const uint32_t* work, const uint32_t* orig_ix, const uint32_t* spell,
                uint64_t n, uint32_t n_works, uint32_t n_script, uint32_t n_spell,
                fs_variant_word* words, fs_variant_cell* cells, uint64_t cap, uint64_t* n_cells);

/* `ao3.py readings`: the wordings fans give each quoted stretch.  Records are sorted by (work,
 * fan_ix), as for fs_passages; each carries spell, a dense id < n_spell for its fan word
 * (fs_matches_intern, or any dense numbering).  Passages are those of fs_passages under
 * min_words and max_gap; a passage is a run of consecutive records.
 *  - The reading of a passage with records r0..r(k-1) is the sequence (orig_ix[ri] -
 *    orig_ix[r0], spell[ri]) for i = 0..k-1, together with orig_ix[r0].
 *  - Two passages have the same reading exactly when these are equal.  Sequences are compared,
 *    never hashes alone.
 *  - Passages with the same reading therefore have the same span (orig_first, orig_last) and
 *    the same length.
 *  - With max_gap > 0, two passages over one span that bridge different words are different
 *    readings.
 * A work that repeats a reading ten times counts once in n_works and ten times in n_passages. */
typedef struct fs_reading {
  uint64_t first;            /* first record of its first passage (record order)        */
  uint32_t orig_first, orig_last;
  uint32_t n_words;          /* records in each of its passages                         */
  uint32_t n_passages;       /* passages with this reading                              */
  uint32_t n_works;          /* distinct works among them                               */
  uint32_t span;             /* index into the spans output                             */
  uint32_t rank;             /* 1.. within its span                                     */
  uint32_t reserved;         /* 0                                                       */
} fs_reading;                /* 40 bytes                                                */

typedef struct fs_reading_span {
  uint32_t orig_first, orig_last;
  uint32_t n_passages, n_works;        /* over all its readings; works distinct         */
  uint32_t n_readings, first_reading;  /* its readings are first_reading .. +n_readings */
} fs_reading_span;           /* 24 bytes                                                */

/* The device tables are open-addressing tables of S slots each, S the power of two that is at
 * least twice the number of passages (and at least 64), FS_READINGS_SLOT_BYTES bytes per slot
 * over all of them: S * FS_READINGS_SLOT_BYTES may be up to FS_READINGS_MAX_BYTES, which
 * admits 2^23 passages. */
#define FS_READINGS_SLOT_BYTES 64u
#define FS_READINGS_MAX_BYTES (1u << 30)

/* Host columns in; `cap_readings` readings and `cap_spans` spans out, on HIP device `device`.
 * Spans are sorted by orig_first ascending, then orig_last ascending.  Readings are in span
 * order; within a span they are sorted by n_works descending, then n_passages descending, then
 * first ascending: a total order, which gives rank.  FS_E_INVALID for min_words == 0, records
 * out of (work, fan_ix) order, a work >= n_works, an orig_ix >= n_script or a spell >= n_spell;
 * FS_E_UNSUPPORTED for n_rows >= 2^32, n_script > FS_WORKS_MAX_SCRIPT or tables above
 * FS_READINGS_MAX_BYTES; FS_E_CAPACITY when either cap is too small (all three counts are
 * filled in then, the buffers untouched).  n_rows == 0: zeros, without device work.  The
 * environment's FS_READINGS_HASH_BITS=k (a diagnostic, read once per call) keeps k bits of the
 * sequence hash, so that at 0 every passage collides; the output is the same.  There is no
 * _rows twin: fs_row carries no fan word, so records a search left on the device cannot feed
 * this. */
int fs_readings(int device, const uint32_t* work, const uint32_t* fan_ix, const uint32_t* orig_ix,
                const uint32_t* spell, uint64_t n_rows, uint32_t n_works, uint32_t n_script,
                uint32_t n_spell, uint32_t min_words, uint32_t max_gap,
                fs_reading* readings, uint64_t cap_readings,
                fs_reading_span* spans, uint64_t cap_spans,
                uint64_t* n_readings, uint64_t* n_spans, uint64_t* n_passages);
/* HIP-event milliseconds of the last fs_readings call on this thread: passages (checks, run
 * heads, kept runs), tables (hashes, inserts and counts), spans (their order and records),
 * readings (their places and ranks), copy out, and the total of the five; 0 for a pass that
 * did not run.  tools/readings_bench.py. */
int fs_readings_times(double* ms);

/* `ao3.py retellings`: works that quote the script in its order.  Records and passages as for
 * fs_passages; inside a work the passages are numbered in record order, and passage k has
 * n_words (its records), fan_first / fan_last and orig_first / orig_last (the fan and the
 * script index of its first and last record).
 *  - Passage i may follow passage j of the same work when j comes before i in record order and
 *    orig_first(i) > orig_last(j): touching at one script word is not following,
 *    orig_last(j) + 1 is.  A chain is a sequence of passages each following the one before; its
 *    weight is the sum of its passages' n_words.
 *  - best(i) = n_words(i) + max(0, max over the j that i may follow of best(j)).
 *  - prev(i) is the j at that maximum, the smallest j on a tie; none when no j qualifies.
 *  - depth(i) = 1 + depth(prev(i)), or 1 without a prev.
 *  - The work's chain ends at the passage with the largest best, the smallest i on a tie, and
 *    is read back through prev.
 *  - A work's descents are the pairs of consecutive passages (k, k + 1) with
 *    orig_first(k + 1) <= orig_last(k); for a work with a passage, n_descents == 0 exactly when
 *    the chain holds all its passages.
 * Every output is an integer below 2^32 (best never exceeds the number of records), and the
 * candidates j are compared as (best(j), ~j), a total order: no schedule changes the result. */
typedef struct fs_retelling {          /* one per work; zeros and 0xFFFFFFFF for a work without a passage */
  uint32_t n_passages, passage_words;  /* as fs_work                                              */
  uint32_t chain_passages, chain_words;
  uint32_t chain_first, chain_last;    /* numbers (in the passage list) of the chain's ends; 0xFFFFFFFF: none */
  uint32_t orig_first, orig_last;      /* orig_first of the chain's first passage, orig_last of its last; 0 without a chain */
  uint32_t chain_script_words;         /* sum of (orig_last - orig_first + 1) over the chain's passages */
  uint32_t n_descents;
} fs_retelling;                        /* 40 bytes                                                */

typedef struct fs_retelling_passage {  /* one per passage of the whole input, in record order     */
  uint64_t first;                      /* index of its first record                               */
  uint32_t n_words, work;
  uint32_t fan_first, fan_last, orig_first, orig_last;
  uint32_t best, prev;                 /* prev: a number in this list, 0xFFFFFFFF: none           */
  uint32_t depth;
  uint32_t chain_pos;                  /* 1-based place in its work's chain, 0 when not in it     */
} fs_retelling_passage;                /* 48 bytes                                                */

/* Host columns in; out[n_works] and `cap` passages out, on HIP device `device`.  Both entry
 * points: FS_E_INVALID for null arguments, min_words == 0, records out of (work, fan_ix) order
 * or a work >= n_works; FS_E_UNSUPPORTED for n_rows >= 2^32; FS_E_CAPACITY with *n_passages =
 * passages required when cap is smaller (out is complete then, passages untouched).
 * n_rows == 0: summaries without a passage, *n_passages = 0 (fs_retellings: without device
 * work).  Any number of passages per work is taken; device memory is a few words per record.
 * The works are handled by passage count: up to FS_RETELLINGS_SMALL (default 8) a lane each,
 * up to FS_RETELLINGS_LDS (default and most 4096) a wave each with its arrays in LDS, beyond
 * that a wave each over global memory.  Both are diagnostics of the environment, read on each
 * call (0: no work takes the class); the output is the same wherever they stand. */
int fs_retellings(int device, const uint32_t* work, const uint32_t* fan_ix,
                  const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works, uint32_t min_words,
                  uint32_t max_gap, fs_retelling* out, fs_retelling_passage* passages,
                  uint64_t cap, uint64_t* n_passages);
/* The same over device-resident fs_row records (16-byte aligned) into device buffers (d_out
 * 4-byte, d_passages 8-byte aligned), on the index's device and stream; returns when they are
 * written. */
int fs_retellings_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                       uint32_t min_words, uint32_t max_gap, fs_retelling* d_out,
                       fs_retelling_passage* d_passages, uint64_t cap, uint64_t* n_passages);
/* HIP-event milliseconds of the last fs_retellings / fs_retellings_rows call on this thread:
 * passages (checks, run heads, kept runs, per-work offsets), bins (the works by class), chains
 * (the recurrence, all classes), trace (the walk back and the per-work records), write (the
 * passage records), and the total of the five; 0 for a pass that did not run.
 * tools/retellings_bench.py. */
int fs_retellings_times(double* ms);

/* `ao3.py companions`: stretches of the script related by the fan works that quote both, the
 * transpose of fs_pairs.  Records, passages, active works (works with a passage; N of them) and
 * the coverage C_w as for fs_pairs.  unit_of[n_script] gives every script word a unit number
 * below n_units, or 0xFFFFFFFF for none; a unit may hold any set of script words.  Work w quotes
 * unit u when C_w holds a word o with unit_of[o] == u (a bridged word counts); M_u is the set of
 * active works quoting u and works(u) = |M_u|.  For units a < b, both = |M_a & M_b|; the pair is
 * kept when both >= min_both and both * 100 >= min_share * min(works(a), works(b)) (the product
 * in 64 bits; min_share a whole percentage, 0..100; exactly at the bound is kept).  Every output
 * is an integer. */
typedef struct fs_companion_unit {
  uint32_t works;            /* |M_u|; 0 for a unit nobody quotes                        */
  uint32_t partners;         /* kept pairs the unit is in                               */
  uint32_t best;             /* the partner with the largest both, the smaller unit
                                number on a tie; 0xFFFFFFFF without partners            */
  uint32_t best_both;        /* its both; 0 without partners                            */
} fs_companion_unit;         /* 16 bytes                                                */

typedef struct fs_companion {
  uint32_t a, b;             /* unit numbers, a < b                                     */
  uint32_t both;             /* active works quoting both                               */
  uint32_t works_a, works_b; /* works(a), works(b)                                      */
  uint32_t first_work;       /* smallest and largest work number (not active number)    */
  uint32_t last_work;        /* among them                                              */
  uint32_t reserved;         /* 0                                                       */
} fs_companion;              /* 32 bytes                                                */

/* The incidence matrix is a row of ceil(N / 64) 64-bit words per unit, the units padded to a
 * multiple of 64: ceil(n_units / 64) * 64 * ceil(N / 64) * 8 bytes may be up to this.  The
 * coverage matrix of fs_pairs is not built. */
#define FS_COMPANIONS_MAX_BYTES (1u << 30)

/* Host columns and the host unit map in; units[n_units] and `cap` pairs out, on HIP device
 * `device`.  The pairs come in (a, b) ascending order.  Both entry points: FS_E_INVALID for
 * min_words == 0, min_both == 0, min_share > 100, records out of (work, fan_ix) order, a work >=
 * n_works, an orig_ix >= n_script or a unit_of entry that is neither below n_units nor
 * 0xFFFFFFFF; FS_E_UNSUPPORTED for n_rows >= 2^32, n_script > FS_WORKS_MAX_SCRIPT or an
 * incidence matrix above FS_COMPANIONS_MAX_BYTES; FS_E_CAPACITY with *n_pairs = pairs required
 * when cap is smaller (units is complete then, pairs untouched).  n_rows == 0 or n_units == 0:
 * units of no works with best 0xFFFFFFFF, *n_pairs = 0 (fs_companions: without device work, the
 * unit map unread). */
int fs_companions(int device, const uint32_t* work, const uint32_t* fan_ix,
                  const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works, uint32_t n_script,
                  const uint32_t* unit_of, uint32_t n_units, uint32_t min_words, uint32_t max_gap,
                  uint32_t min_both, uint32_t min_share, fs_companion_unit* units,
                  fs_companion* pairs, uint64_t cap, uint64_t* n_pairs);
/* The same over device-resident fs_row records (16-byte aligned) and a device-resident unit map
 * of the index's n_script entries into device buffers (16-byte aligned), on the index's device
 * and stream; returns when they are written. */
int fs_companions_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                       const uint32_t* d_unit_of, uint32_t n_units, uint32_t min_words,
                       uint32_t max_gap, uint32_t min_both, uint32_t min_share,
                       fs_companion_unit* d_units, fs_companion* d_pairs, uint64_t cap,
                       uint64_t* n_pairs);
/* HIP-event milliseconds of the last fs_companions / fs_companions_rows call on this thread:
 * incidence matrix (with the row popcounts), count pass (with its scan and the per-unit
 * results), place pass, detail pass; 0 for a pass that did not run.  tools/companions_bench.py. */
int fs_companions_times(double* ms);

/* `ao3.py bundles`: sets of stretches of the script that the same fan works quote, where
 * fs_companions relates them two at a time.  Records, passages, active works (N of them),
 * unit_of[n_script], M_u and works(u) as for fs_companions.  A set S is two or more different
 * units; works(S) = |AND of M_u over S|, the active works quoting every unit of S.  S is frequent
 * when works(S) >= min_all.  Every frequent set of 2 .. max_size units is listed; the frequent
 * sets of max_size + 1 units are mined too, used and not listed.
 *  - extensions(S): the frequent sets with one unit more that hold S.  S is closed when none of
 *    them has works equal to works(S), maximal when extensions is 0.  Both are exact for every
 *    listed size, because level max_size + 1 is mined.
 *  - F_k is the list of the frequent sets of k units, each with its units ascending, in
 *    lexicographic order.  The candidates of level k + 1 are F_k[i] plus the last unit of F_k[j]
 *    for i < j where the two agree in their first k - 1 units, taken in (i, j) order, which is
 *    lexicographic again.  F_2 is the kept pairs of fs_companions under min_both = min_all,
 *    min_share = 0.
 *  - A level with more than FS_BUNDLES_MAX_SETS candidates (F_2: kept pairs) ends the call with
 *    FS_E_UNSUPPORTED before an output is written; the error text names the level and the
 *    count.  The environment's FS_BUNDLES_MAX_SETS, read on each call, replaces the bound (tests).
 * Every output is an integer count, a minimum or an OR and every place a scanned count, so no
 * schedule changes a byte. */
#define FS_BUNDLES_MAX_SIZE 8u
#define FS_BUNDLES_MAX_SETS (1u << 22)
/* What a call keeps in device memory may be up to this: the incidence matrix twice (the tiles
 * of fs_companions and a unit-major copy, ceil(N / 64) rounded up to 4 words a unit), the level
 * lists (k + 4 words a set of k units) and the candidate buffers (24 bytes a set of the level
 * joined and 20 a candidate, of one level at a time). */
#define FS_BUNDLES_MAX_BYTES (1u << 30)
#define FS_BUNDLES_TIMES 32

typedef struct fs_bundle {
  uint32_t units[8];         /* ascending; 0xFFFFFFFF behind the first `size`            */
  uint32_t size;             /* 2 .. max_size                                           */
  uint32_t works;            /* works(S)                                                */
  uint32_t first_work;       /* smallest work number (not active number) among them     */
  uint32_t extensions;       /* frequent sets of size + 1 units holding S               */
  uint32_t closed;           /* 1 or 0                                                  */
  uint32_t reserved[3];      /* 0                                                       */
} fs_bundle;                 /* 64 bytes                                                */

typedef struct fs_bundle_unit {
  uint32_t works;            /* |M_u|                                                   */
  uint32_t sets;             /* listed sets (2 .. max_size units, closed or not) with u */
  uint32_t largest;          /* the largest size among them; 0 without one              */
  uint32_t reserved;         /* 0                                                       */
} fs_bundle_unit;            /* 16 bytes                                                */

typedef struct fs_bundle_level {
  uint32_t size;             /* 2 .. max_size + 1                                       */
  uint32_t frequent;         /* |F_size|                                                */
  uint64_t candidates;       /* joined candidates, before any pruning; size 2: the pairs
                                of units with works(u) >= min_all                       */
  uint32_t closed, maximal;  /* of F_size; 0xFFFFFFFF each for size max_size + 1        */
} fs_bundle_level;           /* 24 bytes                                                */

/* Host columns and the host unit map in; units[n_units], levels[max_size] (sizes 2 ..
 * max_size + 1) and `cap` sets out, on HIP device `device`.  The sets come by size ascending,
 * then lexicographically.  Both entry points: FS_E_INVALID for null arguments, min_words == 0,
 * min_all == 0, max_size outside 2 .. FS_BUNDLES_MAX_SIZE, records out of (work, fan_ix) order,
 * a work >= n_works, an orig_ix >= n_script or a unit_of entry that is neither below n_units nor
 * 0xFFFFFFFF; FS_E_UNSUPPORTED for n_rows >= 2^32, n_script > FS_WORKS_MAX_SCRIPT, tables above
 * FS_BUNDLES_MAX_BYTES (the text names them) or a level above FS_BUNDLES_MAX_SETS, no output
 * written; FS_E_CAPACITY with *n_sets = sets required when cap is smaller (units and levels are
 * complete then, sets untouched).  n_rows == 0 or n_units == 0: units and levels of zeros,
 * *n_sets = 0 (fs_bundles: without device work, the unit map unread).
 * The count pass takes a parent set's extensions piece by piece: 64 extensions are a
 * workgroup's work item, so a parent with a thousand extensions is spread over many CUs.
 * FS_BUNDLES_PRUNE (default 1; 0: off), a diagnostic of the environment read on each call,
 * drops a candidate before the count when one of its other subsets of the parent's size is not
 * frequent; the output is the same wherever it stands. */
int fs_bundles(int device, const uint32_t* work, const uint32_t* fan_ix, const uint32_t* orig_ix,
               uint64_t n_rows, uint32_t n_works, uint32_t n_script, const uint32_t* unit_of,
               uint32_t n_units, uint32_t min_words, uint32_t max_gap, uint32_t min_all,
               uint32_t max_size, fs_bundle_unit* units, fs_bundle_level* levels,
               fs_bundle* sets, uint64_t cap, uint64_t* n_sets);
/* The same over device-resident fs_row records (16-byte aligned) and a device-resident unit map
 * of the index's n_script entries into device buffers (d_units and d_sets 16-byte, d_levels
 * 8-byte aligned), on the index's device and stream; returns when they are written. */
int fs_bundles_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                    const uint32_t* d_unit_of, uint32_t n_units, uint32_t min_words,
                    uint32_t max_gap, uint32_t min_all, uint32_t max_size,
                    fs_bundle_unit* d_units, fs_bundle_level* d_levels, fs_bundle* d_sets,
                    uint64_t cap, uint64_t* n_sets);
/* HIP-event milliseconds of the last fs_bundles / fs_bundles_rows call on this thread,
 * ms[0 .. FS_BUNDLES_TIMES): [0] incidence (with the row popcounts and the unit-major copy), [1]
 * level 2 (count, scan, place, first works); for the level of size s = 3 .. 9 at [2 + 4 (s - 3)]:
 * join (with the scans and the candidates' parents and pruning), count, place (with its scan and
 * the first works), mark; [30] the tally and the records; [31] the total of all before it.  0
 * for a pass that did not run.  tools/bundles_bench.py. */
int fs_bundles_times(double* ms);

/* `ao3.py routes`: sequences of stretches of the script that the fan works quote in that order,
 * the ordered counterpart of fs_bundles, where fs_transitions relates the units one step at a
 * time.  Records, passages (min_words, max_gap), unit_of[n_script] and n_units as for
 * fs_transitions; a passage's unit is unit_of[orig_first], and a passage without a unit is left
 * out before anything else.
 *  - Sequence: a work's unit-bearing passages in record order, consecutive passages of one unit
 *    written once; in s_1 .. s_m neighbours always differ.  A work with m < 2 supports no route.
 *  - Route: P = (a_1 .. a_k), 2 <= k <= max_length, a_i != a_i+1; a unit may come back.
 *  - A work supports P when there are p_1 < ... < p_k with s_{p_i} = a_i and p_i+1 - p_i <=
 *    max_skip + 1 for every i.  max_skip is 0 .. FS_ROUTES_MAX_SKIP elements of the sequence
 *    between two units of the route (0: a contiguous run), or 0xFFFFFFFF for any distance.
 *  - works(P) is the number of supporting works; P is frequent when works(P) >= min_all.
 *  - F_1 is the units u with works(u) >= min_all, works(u) counting the works with m >= 2 whose
 *    sequence holds u.  F_k is kept in lexicographic order.  The candidates of level k + 1 are
 *    F_k[i] plus the last unit of F_k[j] for every j whose first k - 1 units are the last k - 1
 *    of F_k[i] (k = 1: every ordered pair of different frequent units); those j are one
 *    contiguous range, so candidates in (i, j) order are lexicographic again.  The join is
 *    complete under every max_skip, because a contiguous part of a supported route is supported;
 *    nothing else is pruned, because under a bounded skip dropping a middle unit does not keep
 *    support.
 *  - Levels 2 .. max_length + 1 are mined, 2 .. max_length listed.  forward(P): the frequent
 *    routes P + b; backward(P): the frequent routes a + P; P is closed when none of those has
 *    works equal to works(P), exact for every listed length.  prefix_works(P): the works of P
 *    without its last unit (k = 2: works(a_1)).
 *  - A level with more than FS_ROUTES_MAX_SETS candidates ends the call with FS_E_UNSUPPORTED
 *    before an output is written; the error text names the level and the count.  The
 *    environment's FS_ROUTES_MAX_SETS, read on each call, replaces the bound (tests).
 * Every output is an integer count, a minimum or an OR and every place a scanned count, so no
 * schedule changes a byte. */
#define FS_ROUTES_MAX_LENGTH 8u
#define FS_ROUTES_MAX_SKIP 63u
#define FS_ROUTES_MAX_SETS (1u << 22)
/* What a call keeps in device memory may be up to this.  With E the elements of all sequences
 * of two or more and a row ceil(E / 64) 64-bit words: the heads, the tails, the unit and the
 * work of every position, the set behind works(u) and a row per frequent unit; a row per route
 * of two adjacent levels at a time; the level lists (k + 8 words a route of k units) and the
 * candidate buffers (28 bytes a route of the level joined, 12 a slice of its rows and 16 a
 * candidate, of one level at a time). */
#define FS_ROUTES_MAX_BYTES (1u << 30)
#define FS_ROUTES_TIMES 43

typedef struct fs_route {
  uint32_t units[8];         /* in route order; 0xFFFFFFFF behind the first `length`     */
  uint32_t length;           /* 2 .. max_length                                         */
  uint32_t works;            /* works(P)                                                */
  uint32_t first_work;       /* smallest supporting work number                         */
  uint32_t prefix_works;     /* works of P without its last unit                        */
  uint32_t forward;          /* frequent routes P + b                                   */
  uint32_t backward;         /* frequent routes a + P                                   */
  uint32_t closed;           /* 1 or 0                                                  */
  uint32_t reserved;         /* 0                                                       */
} fs_route;                  /* 64 bytes                                                */

typedef struct fs_route_unit {
  uint32_t works;            /* works with m >= 2 whose sequence holds u                */
  uint32_t routes;           /* listed routes (closed or not) holding u, each once      */
  uint32_t longest;          /* the largest length among them; 0 without one            */
  uint32_t reserved;         /* 0                                                       */
} fs_route_unit;             /* 16 bytes                                                */

typedef struct fs_route_level {
  uint32_t length;           /* 2 .. max_length + 1                                     */
  uint32_t frequent;         /* |F_length|                                              */
  uint64_t candidates;       /* joined candidates                                       */
  uint32_t closed;           /* of F_length; 0xFFFFFFFF for length max_length + 1       */
  uint32_t reserved;         /* 0                                                       */
} fs_route_level;            /* 24 bytes                                                */

/* Host columns and the host unit map in; units[n_units], levels[max_length] (lengths 2 ..
 * max_length + 1) and `cap` routes out, on HIP device `device`.  The routes come by length
 * ascending, then lexicographically.  Both entry points: FS_E_INVALID for null arguments,
 * min_words == 0, min_all == 0, max_length outside 2 .. FS_ROUTES_MAX_LENGTH, max_skip in
 * FS_ROUTES_MAX_SKIP + 1 .. 0xFFFFFFFE, records out of (work, fan_ix) order, a work >= n_works,
 * an orig_ix >= n_script or a unit_of entry that is neither below n_units nor 0xFFFFFFFF;
 * FS_E_UNSUPPORTED for n_rows >= 2^32, n_script > FS_WORKS_MAX_SCRIPT, tables above
 * FS_ROUTES_MAX_BYTES (the text names them) or a level above FS_ROUTES_MAX_SETS, no output
 * written; FS_E_CAPACITY with *n_routes = routes required when cap is smaller (units and levels
 * are complete then, routes untouched).  n_rows == 0 or n_units == 0: units and levels of
 * zeros, *n_routes = 0 (fs_routes: without device work, the unit map unread).
 * The rows are stepped and counted in slices of FS_ROUTES_SLICE_WORDS 64-bit words (default and
 * most 256), a diagnostic of the environment read on each call; a work whose sequence spans
 * slices is carried across them, and the output is the same wherever it stands.  The count pass
 * takes a route's extensions piece by piece, 64 a workgroup's work item. */
int fs_routes(int device, const uint32_t* work, const uint32_t* fan_ix, const uint32_t* orig_ix,
              uint64_t n_rows, uint32_t n_works, uint32_t n_script, const uint32_t* unit_of,
              uint32_t n_units, uint32_t min_words, uint32_t max_gap, uint32_t max_skip,
              uint32_t min_all, uint32_t max_length, fs_route_unit* units,
              fs_route_level* levels, fs_route* routes, uint64_t cap, uint64_t* n_routes);
/* The same over device-resident fs_row records (16-byte aligned) and a device-resident unit map
 * of the index's n_script entries into device buffers (d_units and d_routes 16-byte, d_levels
 * 8-byte aligned), on the index's device and stream; returns when they are written. */
int fs_routes_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                   const uint32_t* d_unit_of, uint32_t n_units, uint32_t min_words,
                   uint32_t max_gap, uint32_t max_skip, uint32_t min_all, uint32_t max_length,
                   fs_route_unit* d_units, fs_route_level* d_levels, fs_route* d_routes,
                   uint64_t cap, uint64_t* n_routes);
/* HIP-event milliseconds of the last fs_routes / fs_routes_rows call on this thread,
 * ms[0 .. FS_ROUTES_TIMES): [0] the sequence, the positions and the rows of the units; for the
 * level of length l = 2 .. 9 at [1 + 5 (l - 2)]: join, step, count, place (with its scan, the
 * rows and the first works), mark; [41] the tally and the records; [42] the total of all before
 * it.  0 for a pass that did not run.  tools/routes_bench.py. */
int fs_routes_times(double* ms);

/* `ao3.py lines`: the lines of the script by how completely the fan works quote them.  Records,
 * passages, active works (works with a passage; N of them, numbered in work order) and the
 * coverage C_w as for fs_pairs.  line_first[n_lines + 1] cuts the script into lines: line l owns
 * the script words line_first[l] .. line_first[l + 1] - 1, line_first[0] = 0 and
 * line_first[n_lines] = n_script, strictly ascending (no empty line).  A cell (l, w) exists when
 * C_w holds a word of line l; covered = the words of the line in C_w, first and last the smallest
 * and largest of them, runs the maximal stretches of consecutive ones; the cell is whole when
 * covered = the words of the line.  Every output is an integer. */
typedef struct fs_line {
  uint32_t works;            /* cells of the line                                        */
  uint32_t whole_works;      /* whole ones among them                                    */
  uint32_t most_works;       /* cells with covered * 100 >= most * words (64 bits;
                                exactly at the bound counts, whole cells count)          */
  uint32_t head_works;       /* cells holding the line's first word                      */
  uint32_t tail_works;       /* cells holding its last word                              */
  uint32_t first_work;       /* smallest work number with a cell; 0xFFFFFFFF without     */
  uint64_t covered_sum;      /* covered summed over the cells                            */
} fs_line;                   /* 32 bytes                                                 */

typedef struct fs_line_work {
  uint32_t work;             /* work number of this active work                          */
  uint32_t lines;            /* cells of the work                                        */
  uint32_t whole_lines;      /* whole ones among them                                    */
  uint32_t covered;          /* covered summed over its cells = |C_w|                    */
  uint32_t line_words;       /* the words of the lines it has a cell in                  */
  uint32_t top_line;         /* the line with the largest covered, the earlier on a tie  */
  uint32_t top_covered;      /* its covered                                              */
  uint32_t reserved;         /* 0                                                        */
} fs_line_work;              /* 32 bytes                                                 */

typedef struct fs_line_cell {
  uint32_t line;             /* line number                                              */
  uint32_t work;             /* work number (not active number)                          */
  uint32_t covered;          /* words of the line in C_w, >= 1                           */
  uint32_t first, last;      /* smallest and largest of them (script word indices)       */
  uint32_t runs;             /* maximal runs of consecutive covered words in the line    */
  uint32_t reserved;         /* 0                                                        */
  uint32_t reserved2;        /* 0                                                        */
} fs_line_cell;              /* 32 bytes                                                 */

/* Counted: the coverage, a 64-bit word per 64 script words and active work with the active works
 * padded to a multiple of 64 (ceil(n_script / 64) * ceil(N / 64) * 64 * 8 bytes), and, per line
 * and column of 64 active works, the incidence word and the cells in front of the column
 * (n_lines * ceil(N / 64) * 12 bytes).  Their sum may be up to this. */
#define FS_LINES_MAX_BYTES (1u << 30)

/* Host columns and the host line table in; lines[n_lines], up to works_cap active works in
 * active order and up to cells_cap cells in (line, work) order out, on HIP device `device`.
 * Both entry points: FS_E_INVALID for min_words == 0, most outside 1..100, records out of (work,
 * fan_ix) order, a work >= n_works, an orig_ix >= n_script or a line_first that is not strictly
 * ascending from 0 to n_script; FS_E_UNSUPPORTED for n_rows >= 2^32, n_script >
 * FS_WORKS_MAX_SCRIPT or tables above FS_LINES_MAX_BYTES; FS_E_CAPACITY with *n_active and
 * *n_cells = the counts required when either cap is smaller (lines is complete then, works and
 * cells untouched).  n_rows == 0 or n_lines == 0: lines of no works with first_work 0xFFFFFFFF,
 * *n_active = *n_cells = 0 (fs_lines: without device work, the line table unread). */
int fs_lines(int device, const uint32_t* work, const uint32_t* fan_ix, const uint32_t* orig_ix,
             uint64_t n_rows, uint32_t n_works, uint32_t n_script, const uint32_t* line_first,
             uint32_t n_lines, uint32_t min_words, uint32_t max_gap, uint32_t most,
             fs_line* lines, fs_line_work* works, uint64_t works_cap, uint64_t* n_active,
             fs_line_cell* cells, uint64_t cells_cap, uint64_t* n_cells);
/* The same over device-resident fs_row records (16-byte aligned) and a device-resident line
 * table of n_lines + 1 entries into device buffers (16-byte aligned), n_script taken from the
 * index, on the index's device and stream; returns when they are written. */
int fs_lines_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                  const uint32_t* d_line_first, uint32_t n_lines, uint32_t min_words,
                  uint32_t max_gap, uint32_t most, fs_line* d_lines, fs_line_work* d_works,
                  uint64_t works_cap, uint64_t* n_active, fs_line_cell* d_cells,
                  uint64_t cells_cap, uint64_t* n_cells);
/* HIP-event milliseconds of the last fs_lines / fs_lines_rows call on this thread: tables
 * (coverage, incidence, the cell offsets), walk (with the per-work records), and their total; 0
 * for a pass that did not run.  tools/lines_bench.py. */
int fs_lines_times(double* ms);

/* `ao3.py fragments`: the phrases the fan works quote word for word, the closed frequent
 * intervals of the script.  Records, passages, active works (N of them, numbered in work order)
 * and the coverage C_w as for fs_pairs: every script word from a passage's first record to its
 * last, bridged words included, a word quoted twice once.
 *  - A run of a work is a maximal stretch of consecutive script words in C_w; passages of one
 *    work that abut or overlap make one run.  A work holds [a, b] when one of its runs contains
 *    it.  S(a, b) is the number of active works holding [a, b]; 0 outside the script.
 *  - [a, b] of k = b - a + 1 words is a fragment when min_length <= k <= max_words, S(a, b) >=
 *    min_works, and it is closed: S(a, b) > S(a - 1, b) and S(a, b) > S(a, b + 1).  Closedness
 *    looks at every length: a stretch of max_words words whose extension has the same support is
 *    no fragment, and a fragment longer than max_words is not listed.  Runs longer than max_words
 *    count for every interval inside them.
 * Every output is an integer: sums and minima, places from scanned counts. */
typedef struct fs_fragment {
  uint32_t first, last;      /* script word indices                                      */
  uint32_t works;            /* S(first, last)                                           */
  uint32_t exact_works;      /* runs that are exactly [first, last]                      */
  uint32_t start_works;      /* runs starting at first and reaching last = S(first, last)
                                - S(first - 1, last), >= 1                               */
  uint32_t end_works;        /* runs ending at last that hold first = S(first, last) -
                                S(first, last + 1), >= 1                                 */
  uint32_t first_work;       /* smallest work number with a run counted in start_works   */
  uint32_t reserved;         /* 0                                                        */
} fs_fragment;               /* 32 bytes                                                 */

typedef struct fs_fragment_work {
  uint32_t work;             /* work number of this active work                          */
  uint32_t runs;             /* its runs                                                 */
  uint32_t covered;          /* |C_w|                                                    */
  uint32_t held;             /* listed fragments inside one of its runs (modulo 2^32)    */
  uint32_t exact;            /* its runs that are themselves listed fragments            */
  uint32_t longest_first;    /* its longest run, the first among equals                  */
  uint32_t longest_last;
  uint32_t longest_works;    /* S of that run; 0xFFFFFFFF when its length is outside
                                [min_length, max_words]                                  */
} fs_fragment_work;          /* 32 bytes                                                 */

#define FS_FRAGMENTS_MAX_WORDS 4096u
/* Counted: the coverage (ceil(n_script / 64) * ceil(N / 64) * 64 * 8 bytes), the run list (12
 * bytes per passage of the records, kept or not, and with the dedupe 16 bytes per slot of its
 * table, the power of two at or above twice that number), and four tables (runs starting, runs
 * ending, first work, exact runs) of (min(max_words, n_script) - min_length + 1) * n_script
 * 32-bit words each.  Their sum may be up to this. */
#define FS_FRAGMENTS_MAX_BYTES (1u << 30)

/* Host columns in; up to frags_cap fragments in (words, first) ascending order and up to
 * works_cap active works in active order out, on HIP device `device`.  Both entry points:
 * FS_E_INVALID for null arguments, min_words == 0, min_length == 0, max_words < min_length,
 * records out of (work, fan_ix) order, a work >= n_works or an orig_ix >= n_script;
 * FS_E_UNSUPPORTED for max_words > FS_FRAGMENTS_MAX_WORDS, n_rows >= 2^32, n_script >
 * FS_WORKS_MAX_SCRIPT or tables above FS_FRAGMENTS_MAX_BYTES (the message names both factors of
 * a table and says to lower max_words); FS_E_CAPACITY with *n_frags and *n_active = the counts
 * required when either cap is smaller (both buffers untouched then).  n_rows == 0: both counts
 * 0, without device work.
 * Diagnostics of the environment, read on each call; the output is the same wherever they
 * stand:
 *   FS_FRAGMENTS_DEDUP      1 (default): the runs are reduced to the distinct (first, last) with
 *                           a count and a smallest work before they are spread over the tables;
 *                           0: every run is spread by itself
 *   FS_FRAGMENTS_HASH_BITS  keeps that many bits of the hash behind the dedupe (0: every key
 *                           probes from slot 0) */
int fs_fragments(int device, const uint32_t* work, const uint32_t* fan_ix,
                 const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works, uint32_t n_script,
                 uint32_t min_words, uint32_t max_gap, uint32_t min_works, uint32_t min_length,
                 uint32_t max_words, fs_fragment* frags, uint64_t frags_cap, uint64_t* n_frags,
                 fs_fragment_work* works, uint64_t works_cap, uint64_t* n_active);
/* The same over device-resident fs_row records (16-byte aligned) into device buffers (16-byte
 * aligned), n_script taken from the index, on the index's device and stream; returns when they
 * are written. */
int fs_fragments_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                      uint32_t min_words, uint32_t max_gap, uint32_t min_works,
                      uint32_t min_length, uint32_t max_words, fs_fragment* d_frags,
                      uint64_t frags_cap, uint64_t* n_frags, fs_fragment_work* d_works,
                      uint64_t works_cap, uint64_t* n_active);
/* HIP-event milliseconds of the last fs_fragments / fs_fragments_rows call on this thread: runs
 * (coverage and the run list), spread (the dedupe and the tables), list (both row scans and the
 * offsets between them), works (held fragments, the per-work records), and the total
 * of the four; 0 for a pass that did not run.  tools/fragments_bench.py. */
int fs_fragments_times(double* ms);

/* `ao3.py digest`: the fewest works that show what the fan works quote, greedy maximum coverage.
 * Records, passages, active works (N of them, numbered in work order) and the coverage C_w as
 * for fs_pairs.  U is the union of every C_w and TOTAL = |U|.
 *  - K_0 is empty.  In round r = 1, 2, ... gain_r(w) = |C_w \ K_{r-1}|; the pick p_r is the
 *    active work with the largest gain, the smaller work number on a tie; K_r = K_{r-1} | C_{p_r},
 *    and every word of C_{p_r} \ K_{r-1}, the new words of the pick, gets the stamp r.
 *  - Tested before pick r is made: stop when max_picks != 0 and r - 1 == max_picks; when the
 *    largest gain is below min_gain; when |K_{r-1}| * 100 >= cover * TOTAL (64 bits; exactly at
 *    the bound stops).  With max_picks 0, cover 100 and min_gain 1 the rounds end at K = U.  R,
 *    the picks made, is at most min(N, TOTAL).
 * Every output is an integer. */
typedef struct fs_digest_pick {
  uint32_t work;             /* work number of the pick; record r - 1 is pick r          */
  uint32_t covered;          /* |C_w|                                                    */
  uint32_t new_words;        /* its gain, >= min_gain                                    */
  uint32_t new_runs;         /* maximal runs of consecutive new words                    */
  uint32_t longest_first;    /* the longest of them, the first among equals: its first   */
  uint32_t longest_words;    /* script word and its length                               */
  uint32_t cum_words;        /* |K_r|                                                    */
  uint32_t reserved;         /* 0                                                        */
} fs_digest_pick;            /* 32 bytes                                                 */

typedef struct fs_digest_work {
  uint32_t work;             /* work number of this active work                          */
  uint32_t covered;          /* |C_w|                                                    */
  uint32_t pick_rank;        /* r when it is pick r; 0xFFFFFFFF when it was not picked   */
  uint32_t in_picks;         /* |C_w & K_R|                                              */
  uint32_t subsumed_at;      /* the largest stamp over C_w when K_R holds all of C_w: the
                                fewest first picks that show all it quotes; else
                                0xFFFFFFFF                                               */
  uint32_t best_pick;        /* the rank of the pick sharing most words with it, the
                                earlier pick on a tie; 0xFFFFFFFF when none shares one   */
  uint32_t best_shared;      /* |C_w & C_pick| of that pick; 0 without                   */
  uint32_t reserved;         /* 0                                                        */
} fs_digest_work;            /* 32 bytes                                                 */

/* Counted: the coverage matrix (ceil(n_script / 64) * ceil(N / 64) * 64 * 8 bytes), the rows of
 * the picks gathered for the best-pick pass (the same per 64 picks, for min(N, n_script) picks or
 * max_picks if that is fewer), and the arrays per work (16 bytes), per 64 script words (272
 * bytes) and per pick (32 bytes).  Their sum may be up to this. */
#define FS_DIGEST_MAX_BYTES (1u << 30)

/* Host columns in; the R picks in pick order, the N active works in active order and TOTAL out,
 * on HIP device `device`.  Both entry points: FS_E_INVALID for null arguments, min_words == 0,
 * min_gain == 0, cover outside 1..100, records out of (work, fan_ix) order, a work >= n_works or
 * an orig_ix >= n_script; FS_E_UNSUPPORTED for n_rows >= 2^32, n_script > FS_WORKS_MAX_SCRIPT or
 * tables above FS_DIGEST_MAX_BYTES (the message names the three parts); FS_E_CAPACITY with
 * *n_picks and *n_active = the counts required when either cap is smaller (both buffers untouched
 * then; *total_words is set).  n_rows == 0: all three counts 0, without device work.
 * Diagnostics of the environment, read on each call; the output is the same wherever they
 * stand:
 *   FS_DIGEST_LAZY   1 (default): a tile of 64 works is left unread in a round when the largest
 *                    gain its works had when last computed is below the gain already found; 0:
 *                    every tile with a work left is read in every round
 *   FS_DIGEST_SEED_TILES  the next round's best is seeded, with the recomputed gain of the work
 *                    that had the largest gain when last computed, above this many tiles of 64
 *                    active works, default 256; below, every tile's workgroup runs at once and
 *                    a tile left unread shortens no round
 *   FS_DIGEST_BATCH  rounds enqueued between two looks at the device's done word, default 64
 *   FS_DIGEST_COUNT  1: the tiles read are counted (fs_digest_times) */
int fs_digest(int device, const uint32_t* work, const uint32_t* fan_ix, const uint32_t* orig_ix,
              uint64_t n_rows, uint32_t n_works, uint32_t n_script, uint32_t min_words,
              uint32_t max_gap, uint32_t max_picks, uint32_t cover, uint32_t min_gain,
              fs_digest_pick* picks, uint64_t picks_cap, uint64_t* n_picks,
              fs_digest_work* works, uint64_t works_cap, uint64_t* n_active,
              uint64_t* total_words);
/* The same over device-resident fs_row records (16-byte aligned) into device buffers (16-byte
 * aligned), n_script taken from the index, on the index's device and stream; returns when they
 * are written. */
int fs_digest_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                   uint32_t min_words, uint32_t max_gap, uint32_t max_picks, uint32_t cover,
                   uint32_t min_gain, fs_digest_pick* d_picks, uint64_t picks_cap,
                   uint64_t* n_picks, fs_digest_work* d_works, uint64_t works_cap,
                   uint64_t* n_active, uint64_t* total_words);
/* Six numbers of the last fs_digest / fs_digest_rows call on this thread.  HIP-event
 * milliseconds: coverage (with the union and the first bounds), rounds (every batch and the
 * host's looks between them), works (the best-pick product and the per-work records), and the
 * total of the three; 0 for a pass that did not run.  Then the rounds enqueued, and the tiles
 * the gain pass read in them (0 unless FS_DIGEST_COUNT=1).  tools/digest_bench.py. */
int fs_digest_times(double* ms);

/* `ao3.py intervals`: how sure the works-per-unit counts are, a Poisson bootstrap over the fan
 * works.  Records, passages, active works (N of them, numbered in work order), the coverage
 * C_w, unit_of[n_script], M_u and works(u) as for fs_companions.  n_works is every work of the
 * file, active or not.  For replicate b (0-based, b < replicates) and work w (its work number)
 *     z = ((b << 32) | w) + seed * 0x9E3779B97F4A7C15                  (mod 2^64)
 *     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *     z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *     z =  z ^ (z >> 31);  h = z >> 32
 *     m(b, w) = the number of k in 0..12 with h >= T[k],
 *     T[k] = floor(2^32 * sum_{i <= k} e^-1 / i!), the Poisson(1) distribution function:
 *     1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777,
 *     4294923276, 4294962463, 4294966817, 4294967252, 4294967292, 4294967295
 * so a multiplicity is at most 13 and a pure function of (seed, b, w).  Per replicate:
 * N_b = the sum of m(b, w) over all n_works works, A_b the same over the active works,
 * c_b(u) = the sum of m(b, w) over M_u, ppm_b(u) = c_b(u) * 1000000 / max(1, N_b) (64 bits,
 * rounded down), Q_b = the units with c_b(u) > 0.  Per unit, with s the c_b(u) in ascending
 * order and t = replicates * (100 - level) / 200 (rounded down): low = s[t], high =
 * s[replicates - 1 - t], median = s[(replicates - 1) / 2]; the same three over the ppm_b(u),
 * sorted on their own.  The observed order is works(u) descending, then u ascending; next is the
 * unit behind u in it.  Every output is an integer. */
typedef struct fs_interval_unit {
  uint32_t works;            /* |M_u|                                                     */
  uint32_t works_low;        /* s[t]                                                      */
  uint32_t works_median;     /* s[(replicates - 1) / 2]                                   */
  uint32_t works_high;       /* s[replicates - 1 - t]                                     */
  uint32_t ppm;              /* works * 1000000 / max(1, n_works)                         */
  uint32_t ppm_low;          /* the three order statistics of ppm_b(u)                    */
  uint32_t ppm_median;
  uint32_t ppm_high;
  uint32_t rank;             /* 1 + the units with more works                             */
  uint32_t next;             /* the unit behind this one in the observed order;
                                0xFFFFFFFF for the last, whose three counts are 0         */
  uint32_t ahead;            /* replicates with c_b(u) >  c_b(next)                       */
  uint32_t tied;             /*                        ==                                 */
  uint32_t behind;           /*                        <       ; the three sum to
                                replicates                                                */
  uint32_t reserved;         /* 0                                                         */
  uint64_t mean_milli;       /* (the sum of c_b(u) over b) * 1000 / replicates            */
} fs_interval_unit;          /* 64 bytes                                                  */

typedef struct fs_interval_replicate {
  uint32_t resampled_works;  /* N_b                                                       */
  uint32_t resampled_active; /* A_b                                                       */
  uint32_t units_quoted;     /* Q_b                                                       */
  uint32_t reserved;         /* 0                                                         */
} fs_interval_replicate;     /* 16 bytes                                                  */

#define FS_INTERVALS_MAX_REPLICATES 4096u
#define FS_INTERVALS_MAX_WORKS (1u << 28)   /* n_works up to this: 13 * n_works fits 32 bits */
/* Counted: the incidence matrix (ceil(n_units / 64) * 64 * ceil(N / 64) * 8 bytes), the
 * multiplicity bytes (replicates padded to a multiple of 16, times N padded to a multiple of
 * 64) and the counts c_b(u) (4 bytes per padded unit and padded replicate).  Their sum may be
 * up to this. */
#define FS_INTERVALS_MAX_BYTES (1u << 30)

/* Host columns and the host unit map in; units[n_units] and reps[replicates] out, on HIP device
 * `device`.  Both entry points: FS_E_INVALID for null arguments, min_words == 0, replicates
 * outside 1..FS_INTERVALS_MAX_REPLICATES, level outside 50..99, records out of (work, fan_ix)
 * order, a work >= n_works, an orig_ix >= n_script or a unit_of entry that is neither below
 * n_units nor 0xFFFFFFFF; FS_E_UNSUPPORTED for n_rows >= 2^32, n_script > FS_WORKS_MAX_SCRIPT,
 * n_works > FS_INTERVALS_MAX_WORKS or tables above FS_INTERVALS_MAX_BYTES (the message states
 * the three).  Without an active work every unit has works 0, rank 1, next = the unit behind it
 * and tied = replicates.
 * The passes are separate launches: incidence (fs_companions' own), multiplicities, the product
 * counts[u][b] = sum over w of m(b, w) * M[u][w] on the matrix cores
 * (v_mfma_i32_16x16x64_i8: a 64-bit word of M is one K = 64 step), the order statistics (a
 * workgroup per unit sorts its counts in LDS), and the neighbours (the host sorts works(u)
 * between the two).  Switches of the environment, read once per call; the output is the same
 * wherever they stand:
 *   FS_INTERVALS_MFMA       1 (default): the product by MFMA; 0: a plain integer kernel, a lane
 *                           per (unit, replicate) that walks the set bits of the unit's row
 *   FS_INTERVALS_KSPLIT     the workgroups that share the words of a product tile and add
 *                           their parts; default: 1 from 512 product workgroups on, more
 *                           below, at least 8 words each
 *   FS_INTERVALS_MAX_BYTES  a lower bound than the macro's, for tests */
int fs_intervals(int device, const uint32_t* work, const uint32_t* fan_ix,
                 const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works, uint32_t n_script,
                 const uint32_t* unit_of, uint32_t n_units, uint32_t min_words, uint32_t max_gap,
                 uint32_t replicates, uint64_t seed, uint32_t level, fs_interval_unit* units,
                 fs_interval_replicate* reps);
/* The same over device-resident fs_row records (16-byte aligned) and a device-resident unit map
 * of the index's n_script entries into device buffers (16-byte aligned), on the index's device
 * and stream; returns when they are written. */
int fs_intervals_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                      const uint32_t* d_unit_of, uint32_t n_units, uint32_t min_words,
                      uint32_t max_gap, uint32_t replicates, uint64_t seed, uint32_t level,
                      fs_interval_unit* d_units, fs_interval_replicate* d_reps);
/* HIP-event milliseconds of the last fs_intervals / fs_intervals_rows call on this thread:
 * incidence (with the row popcounts), multiplicities (with N_b and A_b), product, statistics
 * (with Q_b), neighbours (with the host's sort of works(u)), and the total of the five; 0 for a
 * pass that did not run.  tools/intervals_bench.py. */
int fs_intervals_times(double* ms);

/* `ao3.py contrast`: what one set of fan works quotes more than another, a permutation test of
 * every unit at once with the max-statistic correction.  Records, passages, active works, the
 * coverage, unit_of[n_script] and the works quoting a unit as for fs_intervals.  n_works is
 * every work of the file, active or not.  side[n_works] is a byte per work: 0 out, 1 side A,
 * 2 side B.  The pool is the works of side A or B, N = NA + NB of them, active or not.
 * Observed, per unit u: a(u) and b(u) the active works of A and of B quoting u, t = a + b,
 *     D(u)   = a(u) * N - t(u) * NA                      (signed; = a * NB - b * NA)
 *     den(u) = isqrt((t(u) * (N - t(u))) << 20)          (the exact floor of the square root)
 *     X(d,u) = (|d| << 20) / den(u), 0 when den(u) = 0;  X(u) = X(D(u), u)
 * Permutation r (0-based, r < permutations) draws a side A of its own: with h(r, w) the hash of
 * fs_intervals with r in place of the replicate,
 *     z = ((r << 32) | w) + seed * 0x9E3779B97F4A7C15                  (mod 2^64)
 *     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *     z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *     z =  z ^ (z >> 31);  h = z >> 32
 *     key(r, w) = h >> (32 - key_bits), 0 when key_bits = 0
 * side A of r is the NA pool works smallest in (key(r, w), w): exactly NA works, ties on the key
 * to the smaller work number (key_bits = 0: the first NA pool works in every permutation).
 * a_r(u) = the active works of that set quoting u, D_r(u) = a_r(u) * N - t(u) * NA.
 *     GE(u)      = the permutations r with |D_r(u)| >= |D(u)|
 * The family is the units with t(u) >= min_quoting.
 *     MX_r       = the maximum over the family of X(D_r(u), u); 0 with an empty family
 *     MAX_UNIT_r = the first family unit attaining MX_r; 0xFFFFFFFF with an empty family
 *     ADJ_GE(u)  = the permutations r with MX_r >= X(u) for a family unit, 0xFFFFFFFF otherwise
 * Every output is an integer. */
typedef struct fs_contrast_unit {
  uint32_t a_works;          /* a(u)                                                      */
  uint32_t b_works;          /* b(u)                                                      */
  uint32_t ge;               /* GE(u)                                                     */
  uint32_t adj_ge;           /* ADJ_GE(u); 0xFFFFFFFF outside the family                  */
  uint64_t statistic;        /* X(u)                                                      */
  int64_t d;                 /* D(u)                                                      */
} fs_contrast_unit;          /* 32 bytes                                                  */

typedef struct fs_contrast_perm {
  uint64_t max_statistic;    /* MX_r                                                      */
  uint32_t a_active;         /* the active works drawn into side A                        */
  uint32_t max_unit;         /* MAX_UNIT_r                                                */
} fs_contrast_perm;          /* 16 bytes                                                  */

#define FS_CONTRAST_MAX_PERMUTATIONS 4096u
/* n_works up to this, so that every intermediate fits 64 bits: a count is below 2^20 and N at
 * most 2^20, so |D| <= 2^40 and |D| << 20 <= 2^60; t * (N - t) <= 2^38 and, shifted, 2^58. */
#define FS_CONTRAST_MAX_WORKS (1u << 20)
/* Counted: the incidence matrix (ceil(n_units / 64) * 64 * ceil(active works / 64) * 8 bytes),
 * the labels (permutations + 2 rows, padded to a multiple of 64, of ceil(active works / 64) * 8
 * bytes) and the counts (4 bytes per padded unit and padded row of the labels).  Their sum may
 * be up to this. */
#define FS_CONTRAST_MAX_BYTES (1u << 30)

/* Host columns, the host unit map and the host side bytes in; units[n_units] and
 * perms[permutations] out, on HIP device `device`; a_counts is null or
 * [n_units][permutations], a_r(u), the null distribution itself.  Both entry points:
 * FS_E_INVALID for null arguments, min_words == 0, min_quoting == 0, permutations outside
 * 1..FS_CONTRAST_MAX_PERMUTATIONS, key_bits > 32, a side byte above 2, records out of (work,
 * fan_ix) order, a work >= n_works, an orig_ix >= n_script or a unit_of entry that is neither
 * below n_units nor 0xFFFFFFFF; FS_E_UNSUPPORTED for n_rows >= 2^32, n_script >
 * FS_WORKS_MAX_SCRIPT, n_works > FS_CONTRAST_MAX_WORKS or tables above FS_CONTRAST_MAX_BYTES
 * (the message states the three).  No records, no active work, an empty side and an empty pool
 * follow the definitions: every count is 0, so D = 0, GE = permutations, X = 0 and nobody is in
 * the family; without units only perms is written.
 * The passes are separate launches and no workgroup waits on another: incidence (fs_companions'
 * own); selection, a workgroup per permutation: a radix select of the NA-th smallest key over
 * 12 + 12 + 8 bits with histograms in LDS, the hash made again in every pass, the works at the
 * boundary key taken in ascending work number, then the labels of the active works as bits of
 * a matrix L in the layout of M (tiles of 64 permutations, k-major), its last two rows the
 * observed side A and the pool; product, counts[u][r] = sum over k of popc(M[u][k] & L[r][k]),
 * a workgroup per (tile of units, tile of rows of L); the sweeps: a wave per unit for a, b, D,
 * den (a double square root corrected to the exact floor), X, GE and an atomic max into MX_r,
 * then MAX_UNIT_r by an atomic min among the units attaining MX_r together with ADJ_GE(u)
 * against MX in LDS.  Switches of the environment, read once per call; the output is the same
 * wherever they stand:
 *   FS_CONTRAST_PRECHECK   1 (default): a lane reads MX_r first and leaves out an atomic that
 *                          cannot win (MX_r only rises, and every value it takes is a true
 *                          statistic); 0: every atomic is issued.  For the bench
 *   FS_CONTRAST_MAX_BYTES  a lower bound than the macro's, for tests */
int fs_contrast(int device, const uint32_t* work, const uint32_t* fan_ix,
                const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works, uint32_t n_script,
                const uint32_t* unit_of, uint32_t n_units, uint32_t min_words, uint32_t max_gap,
                const uint8_t* side, uint32_t min_quoting, uint32_t permutations, uint64_t seed,
                uint32_t key_bits, fs_contrast_unit* units, fs_contrast_perm* perms,
                uint32_t* a_counts);
/* The same over device-resident fs_row records (16-byte aligned), a device-resident unit map of
 * the index's n_script entries and device-resident side bytes into device buffers (16-byte
 * aligned), on the index's device and stream; returns when they are written. */
int fs_contrast_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                     const uint32_t* d_unit_of, uint32_t n_units, uint32_t min_words,
                     uint32_t max_gap, const uint8_t* d_side, uint32_t min_quoting,
                     uint32_t permutations, uint64_t seed, uint32_t key_bits,
                     fs_contrast_unit* d_units, fs_contrast_perm* d_perms);
/* HIP-event milliseconds of the last fs_contrast / fs_contrast_rows call on this thread:
 * incidence (with the check of the side bytes, the run heads and the numbering of the active
 * works, the host's wait for them included), selection (with the labels), product, sweeps, and
 * the total of the four; 0 for a pass that did not run.  tools/contrast_bench.py. */
int fs_contrast_times(double* ms);
/* The exact floor of the square root of x, as the sweeps compute den(u): a double square root
 * and its correction.  No device is touched. */
uint64_t fs_contrast_isqrt(uint64_t x);

/* `ao3.py trends`: which units the later (or the earlier) fan works quote, every unit tested at
 * once against random re-datings of the same works, with the max-statistic correction of
 * fs_contrast.  Records, passages, active works, the coverage, unit_of[n_script] and the works
 * quoting a unit as for fs_intervals.  n_works is every work of the file, active or not.
 * when[n_works] is 16 bits per work: its period offset x(w), 0 .. FS_TRENDS_MAX_SPAN - 1, or
 * 0xFFFF for a work outside the pool.  The pool is the other works, N of them, active or not,
 * in ascending work number: pool[0 .. N).
 * Observed, per unit u: t(u) the active pool works quoting u, s(u) the sum of their x, X the sum
 * of x over the pool,
 *     D(u)   = s(u) * N - t(u) * X                       (signed; positive: quoted later)
 *     den(u) = isqrt((t(u) * (N - t(u))) << 20)          (fs_contrast_isqrt)
 *     Z(d,u) = (|d| << 10) / den(u), 0 when den(u) = 0;  Z(u) = Z(D(u), u)
 * Re-dating r (0-based, r < permutations) gives every pool work the offset of a pool work drawn
 * uniformly, with replacement: with h(r, w) the hash of fs_intervals (fs_contrast spells it out),
 *     v = (h(r, w) * N) >> 32;   x_r(w) = x(pool[v])
 * s_r(u) sums x_r over the active pool works quoting u, X_r over the pool (it varies with r),
 *     D_r(u)     = s_r(u) * N - t(u) * X_r
 *     GE(u)      = the re-datings r with |D_r(u)| >= |D(u)|
 * The family is the units with t(u) >= min_quoting and t(u) < N.
 *     MX_r       = the maximum over the family of Z(D_r(u), u); 0 with an empty family
 *     MAX_UNIT_r = the first family unit attaining MX_r; 0xFFFFFFFF with an empty family
 *     ADJ_GE(u)  = the re-datings r with MX_r >= Z(u) for a family unit, 0xFFFFFFFF otherwise
 * Every output is an integer. */
typedef struct fs_trends_unit {
  uint32_t quoting;          /* t(u)                                                      */
  uint32_t ge;               /* GE(u)                                                     */
  uint32_t adj_ge;           /* ADJ_GE(u); 0xFFFFFFFF outside the family                  */
  uint32_t first_x;          /* the smallest x among the works of t(u); 0xFFFFFFFF: none  */
  uint32_t last_x;           /* the largest; 0xFFFFFFFF: none                             */
  uint32_t reserved;         /* 0                                                         */
  uint64_t offset_sum;       /* s(u)                                                      */
  uint64_t statistic;        /* Z(u)                                                      */
  int64_t d;                 /* D(u)                                                      */
} fs_trends_unit;            /* 48 bytes                                                  */

typedef struct fs_trends_perm {
  uint64_t max_statistic;    /* MX_r                                                      */
  uint32_t offset_sum;       /* X_r                                                       */
  uint32_t max_unit;         /* MAX_UNIT_r                                                */
} fs_trends_perm;            /* 16 bytes                                                  */

#define FS_TRENDS_MAX_PERMUTATIONS 4096u
/* x(w) is below this: ten bits, two planes of non-negative signed bytes, x & 127 and x >> 7 */
#define FS_TRENDS_MAX_SPAN 1024u
/* n_works up to this, so that every intermediate fits 64 bits: s and X are at most 2^20 * 1023,
 * so |D| <= 2^50 and |D| << 10 <= 2^60; t * (N - t) <= 2^38 and, shifted, 2^58.  A sum of a
 * plane's bytes is below 2^27 (x & 127) and 2^23 (x >> 7): no 32-bit accumulator wraps. */
#define FS_TRENDS_MAX_WORKS (1u << 20)
/* Counted: the incidence matrix (ceil(n_units / 64) * 64 * ceil(active works / 64) * 8 bytes),
 * the two offset planes (permutations + 1 rows, padded to a multiple of 16, of ceil(active
 * works / 64) * 64 bytes, twice) and the sums (4 bytes per padded unit and padded row).  Their
 * sum may be up to this. */
#define FS_TRENDS_MAX_BYTES (1u << 30)

/* Host columns, the host unit map and the host offsets in; units[n_units] and
 * perms[permutations] out, on HIP device `device`; sums is null or [n_units][permutations],
 * s_r(u), the null distribution itself.  Both entry points: FS_E_INVALID for null arguments,
 * min_words == 0, min_quoting == 0, permutations outside 1..FS_TRENDS_MAX_PERMUTATIONS, a `when`
 * from FS_TRENDS_MAX_SPAN on that is not 0xFFFF, records out of (work, fan_ix) order, a work >=
 * n_works, an orig_ix >= n_script or a unit_of entry that is neither below n_units nor
 * 0xFFFFFFFF; FS_E_UNSUPPORTED for n_rows >= 2^32, n_script > FS_WORKS_MAX_SCRIPT, n_works >
 * FS_TRENDS_MAX_WORKS or tables above FS_TRENDS_MAX_BYTES (the message states the three).  No
 * records, no active work and an empty pool follow the definitions: every sum is 0, so D = 0,
 * GE = permutations, Z = 0 and nobody is in the family; without units only perms is written.
 * The passes are separate launches and no workgroup waits on another: the pool (a check of
 * `when`, a scan for the pool positions and N, the pool's offsets in pool order, and the pool as
 * a row of bits over the active works beside fs_companions' incidence); the labels, a lane per
 * (re-dating, work): the hash, the gather, X_r by a workgroup reduction, and for an active work
 * a byte in either plane, re-dating-major, rows padded with zeros to 16 re-datings and 64 works,
 * row `permutations` the observed offsets; the product, s[u][r] = sum over the works w quoting u
 * of lo[r][w] + 128 * hi[r][w], by v_mfma_i32_16x16x64_i8 with one expansion of a word of M from
 * bits to bytes held against both planes; the sweeps: a wave per unit for t, the smallest and
 * largest x, D, den, Z, GE and an atomic max into MX_r (read first, left out where it cannot
 * win), then MAX_UNIT_r by an atomic min among the units attaining MX_r together with ADJ_GE(u)
 * against MX in LDS.  Switches of the environment, read once per call; the output is the same
 * wherever they stand:
 *   FS_TRENDS_MFMA       1 (default): the product by MFMA; 0: a plain integer kernel, a lane per
 *                        (unit, re-dating) that walks the set bits of the unit's row
 *   FS_TRENDS_KSPLIT     the workgroups that share the words of a product tile and add their
 *                        parts; default: 1 from 512 product workgroups on, more below, at least
 *                        8 words each
 *   FS_TRENDS_MAX_BYTES  a lower bound than the macro's, for tests */
int fs_trends(int device, const uint32_t* work, const uint32_t* fan_ix, const uint32_t* orig_ix,
              uint64_t n_rows, uint32_t n_works, uint32_t n_script, const uint32_t* unit_of,
              uint32_t n_units, uint32_t min_words, uint32_t max_gap, const uint16_t* when,
              uint32_t min_quoting, uint32_t permutations, uint64_t seed, fs_trends_unit* units,
              fs_trends_perm* perms, uint32_t* sums);
/* The same over device-resident fs_row records (16-byte aligned), a device-resident unit map of
 * the index's n_script entries and device-resident offsets (2-byte aligned) into device buffers
 * (16-byte aligned), on the index's device and stream; returns when they are written. */
int fs_trends_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                   const uint32_t* d_unit_of, uint32_t n_units, uint32_t min_words,
                   uint32_t max_gap, const uint16_t* d_when, uint32_t min_quoting,
                   uint32_t permutations, uint64_t seed, fs_trends_unit* d_units,
                   fs_trends_perm* d_perms);
/* HIP-event milliseconds of the last fs_trends / fs_trends_rows call on this thread: pool (with
 * the incidence, the run heads and the numbering of the active works, the host's wait for them
 * included), labels, product, sweeps, and the total of the four; 0 for a pass that did not run.
 * tools/trends_bench.py. */
int fs_trends_times(double* ms);

/* `ao3.py neighbours`: each fan work's closest works by the rare script words both quote.
 * Records, passages, coverage C_w and the active works (numbered in work order) as for fs_pairs;
 * N active works.  depth(o) is the number of active works whose coverage holds script word o;
 * weight(o) is 0 where depth(o) == 0, else 1 under FS_NEIGHBOURS_FLAT and the number of bits of
 * N / depth(o) (integer division) under FS_NEIGHBOURS_RARITY: 1 for a word more than half the
 * works cover, at most 32.  score(a, b) is the sum of weight(o) over C_a & C_b (below 2^24),
 * own(a) = score(a, a), ppm(a, b) = score * 1000000 / (own(a) + own(b) - score), rounded down,
 * in 64 bits.  b is a candidate of a when b != a, score >= min_score and ppm >= min_similarity *
 * 10000.  The list of a: its first `top` candidates by the key (ppm << 32) | (0xFFFFFFFF - b),
 * larger first.  Every output is an integer. */
typedef struct fs_neighbour {
  uint32_t a, b;             /* the work and the listed neighbour, work numbers          */
  uint32_t rank;             /* of b in the list of a, from 1                            */
  uint32_t back_rank;        /* of a in the list of b, from 1; 0xFFFFFFFF: not in it     */
  uint32_t ppm;              /* ppm(a, b)                                                */
  uint32_t score;            /* score(a, b)                                              */
  uint32_t shared;           /* |C_a & C_b|                                              */
  uint32_t rarest;           /* the shared script word of largest weight, the first
                                among equals                                             */
  uint32_t rarest_depth;     /* its depth                                                */
  uint32_t rarest_weight;    /* its weight                                               */
  uint32_t run_first;        /* start of the maximal run of consecutive shared script
                                words that holds it                                      */
  uint32_t run_words;        /* its length                                               */
} fs_neighbour;              /* 48 bytes                                                 */

typedef struct fs_neighbour_work {
  uint32_t covered;          /* |C_w|; 0 for a work without a passage                    */
  uint32_t own;              /* own(w)                                                   */
  uint32_t candidates;       /* all candidates, not only the listed ones                 */
  uint32_t listed;           /* entries of its list                                      */
  uint32_t listed_by;        /* works whose list holds it                                */
  uint32_t mutual;           /* listed neighbours whose list holds it                    */
  uint32_t nearest;          /* rank 1; 0xFFFFFFFF without one                           */
  uint32_t nearest_ppm;      /* its ppm; 0 without one                                   */
} fs_neighbour_work;         /* 32 bytes                                                 */

typedef struct fs_neighbour_word {
  uint32_t depth;            /* active works covering the script word                    */
  uint32_t weight;           /* 0 where depth is 0                                       */
} fs_neighbour_word;         /* 8 bytes                                                  */

#define FS_NEIGHBOURS_RARITY 0u
#define FS_NEIGHBOURS_FLAT 1u
#define FS_NEIGHBOURS_MAX_TOP 32u
/* What is counted, with R the active works rounded up to 64, nk = ceil(n_script / 64) and P the
 * partial lists of a row (four per share of the column tiles):
 *   the coverage matrix            R * nk * 8 bytes
 *   the partial lists              R * P * top * 8
 *   their candidate counts         R * P * 4
 *   the lists and the back ranks   R * top * 12
 *   depth and weight               nk * 64 * 5
 *   the words with a bit, by tile  R / 64 * ceil(nk / 64) * 8 */
#define FS_NEIGHBOURS_MAX_BYTES (1u << 30)

/* Host columns in; works[n_works], words[n_script] and `cap` listed pairs out, on HIP device
 * `device`.  The listed pairs come in (a, rank) order.  Both entry points: the FS_E_INVALID and
 * FS_E_UNSUPPORTED cases of fs_pairs (min_score in the place of min_shared, tables above
 * FS_NEIGHBOURS_MAX_BYTES in the place of the matrix), and FS_E_INVALID for a `weight` that is
 * neither FS_NEIGHBOURS_RARITY nor FS_NEIGHBOURS_FLAT, top == 0, top > FS_NEIGHBOURS_MAX_TOP or
 * min_similarity > 100; FS_E_CAPACITY with *n_listed = listed pairs required when cap is
 * smaller (works and words are complete then, the pairs untouched).  n_rows == 0: works without
 * coverage, words without depth, *n_listed = 0 (fs_neighbours: without device work).
 * Environment (diagnostics, read on each call):
 *   FS_NEIGHBOURS_MFMA   0: the product without the matrix instruction (the same results)
 *   FS_NEIGHBOURS_SPLIT  that many shares of the column tiles per stripe of rows, for tests */
int fs_neighbours(int device, const uint32_t* work, const uint32_t* fan_ix,
                  const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works, uint32_t n_script,
                  uint32_t min_words, uint32_t max_gap, uint32_t weight, uint32_t top,
                  uint32_t min_score, uint32_t min_similarity, fs_neighbour_work* works,
                  fs_neighbour_word* words, fs_neighbour* listed, uint64_t cap,
                  uint64_t* n_listed);
/* The same over device-resident fs_row records (16-byte aligned) into device buffers (16-byte
 * aligned), n_script taken from the index, on the index's device and stream; returns when
 * they are written. */
int fs_neighbours_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                       uint32_t min_words, uint32_t max_gap, uint32_t weight, uint32_t top,
                       uint32_t min_score, uint32_t min_similarity, fs_neighbour_work* d_works,
                       fs_neighbour_word* d_words, fs_neighbour* d_listed, uint64_t cap,
                       uint64_t* n_listed);
/* HIP-event milliseconds of the last fs_neighbours / fs_neighbours_rows call on this thread:
 * coverage matrix, depth and weight (with own), product (with the merge of the partial lists),
 * place (back ranks, counts, scan, the works table and the listed pairs), detail, and the total
 * of the five; 0 for a pass that did not run.  tools/neighbours_bench.py. */
int fs_neighbours_times(double* ms);

/* `ao3.py misquotes`: the works that share departures from the script.  Records sorted by
 * (work, fan_ix) with the spelling id of their fan word; passages as for fs_passages; only the
 * records inside a kept passage count, and a work with one is active.  same[o] is the spelling
 * that is script word o itself (0xFFFFFFFF: none).  readers(o): the works with a record at o.
 * A departure is a record whose spelling is not same(o); a misquote m is a pair (o, spelling)
 * with a departure, records(m) its departures, works(m) the works among them.  m is listed when
 * works(m) >= min_works, and numbered among the listed ones by orig_ix ascending, works
 * descending, records descending, spell ascending.  A listed m is telling when works(m) * 100 <=
 * max_share * readers(o) (in 64 bits); its weight is then 1 under FS_MISQUOTES_FLAT and the
 * number of bits of readers(o) / works(m) (integer division) under FS_MISQUOTES_RARITY, and 0
 * when it is not telling.  For works a < b, shared(a, b) is the number of telling misquotes both
 * have and score(a, b) the sum of their weights; the pair is kept when shared >= min_shared and
 * score >= min_score.  Every output is an integer. */
typedef struct fs_misquote {
  uint32_t orig_ix;          /* the script word                                          */
  uint32_t spell;            /* what was written in its place                            */
  uint32_t records;          /* departures                                               */
  uint32_t works;            /* different works among them                               */
  uint32_t readers;          /* readers(orig_ix)                                         */
  uint32_t telling;          /* 1 or 0                                                   */
  uint32_t weight;           /* 0 when not telling                                       */
  uint32_t first_work;       /* the smallest work number that has it                     */
} fs_misquote;               /* 32 bytes                                                 */

typedef struct fs_misquote_pair {
  uint32_t a, b;             /* work numbers, a < b                                      */
  uint32_t shared;           /* telling misquotes both have                              */
  uint32_t score;            /* the sum of their weights                                 */
  uint32_t a_on_common;      /* telling misquotes of a at script words b reads           */
  uint32_t b_on_common;      /* telling misquotes of b at script words a reads           */
  uint32_t strongest;        /* the shared misquote of largest weight (its number), the
                                smallest number among equals                             */
  uint32_t strongest_weight; /* its weight                                               */
} fs_misquote_pair;          /* 32 bytes                                                 */

typedef struct fs_misquote_work {
  uint32_t passage_records;  /* records inside kept passages; 0: not active              */
  uint32_t departures;       /* those that are departures                                */
  uint32_t misquotes;        /* listed misquotes it has                                  */
  uint32_t telling;          /* telling misquotes it has                                 */
  uint32_t singular;         /* misquotes only it has, works(m) == 1                     */
  uint32_t partners;         /* kept pairs it is in                                      */
  uint32_t closest;          /* the partner of largest score, the smallest work number
                                among equals; 0xFFFFFFFF without a partner               */
  uint32_t closest_score;    /* that score; 0 without a partner                          */
} fs_misquote_work;          /* 32 bytes                                                 */

#define FS_MISQUOTES_RARITY 0u
#define FS_MISQUOTES_FLAT 1u
/* What is counted.  P is the number of contributions, the sum of k * (k - 1) / 2 over the
 * telling misquotes with k = works(m), N the active works:
 *   the pair table     S slots of FS_MISQUOTES_SLOT_BYTES: key 8, shared 4, score 4,
 *                      strongest 8, its place among the kept pairs 8; S the power of two at
 *                      least twice min(P, N * (N - 1) / 2) and at least 64
 *   the record tables  R slots of FS_MISQUOTES_RECORD_SLOT_BYTES: the keys (o, work),
 *                      (o, spell) and (misquote, work), 8 each, and records, works, first work
 *                      and number of the misquote in the slot, 4 each; R the power of two at
 *                      least twice n_rows and at least 64
 * Either may take FS_MISQUOTES_MAX_BYTES, which admits 2^24 contributions; beyond that the
 * call is refused before the table is allocated. */
#define FS_MISQUOTES_SLOT_BYTES 32u
#define FS_MISQUOTES_RECORD_SLOT_BYTES 40u
#define FS_MISQUOTES_MAX_BYTES (1u << 30)

/* Host columns in; works[n_works] (always complete: zeros and closest = 0xFFFFFFFF for a work
 * without a passage), up to cap_m listed misquotes in the order of their numbers and up to
 * cap_p kept pairs in (a, b) order out, on HIP device `device`.  FS_E_CAPACITY when either cap
 * is too small: *n_misquotes and *n_pairs say what is required, works is complete, the other
 * two buffers are untouched.  FS_E_INVALID: records not sorted by (work, fan_ix); a work >=
 * n_works, an orig_ix >= n_script, a spell >= n_spell; a same[o] that is neither 0xFFFFFFFF nor
 * below n_spell; min_words == 0, min_works < 2, max_share outside 1 .. 100, min_shared == 0,
 * min_score == 0, a `weight` that is neither FS_MISQUOTES_RARITY nor FS_MISQUOTES_FLAT.
 * FS_E_UNSUPPORTED: n_rows >= 2^27 (a score is 32 bits and a weight at most 32), n_script >
 * FS_WORKS_MAX_SCRIPT, tables above the bound (the message names P and --max-share).
 * n_rows == 0: works without passages, no misquotes, no pairs, without device work.
 * Environment (diagnostics, read once per call):
 *   FS_MISQUOTES_MAX_PAIRS  the most contributions P a call takes; it only lowers the bound
 *   FS_MISQUOTES_HASH_BITS  k bits of every table's hash are kept; at 0 every key collides and
 *                           the output is the same */
int fs_misquotes(int device, const uint32_t* work, const uint32_t* fan_ix,
                 const uint32_t* orig_ix, const uint32_t* spell, const uint32_t* same,
                 uint64_t n_rows, uint32_t n_works, uint32_t n_script, uint32_t n_spell,
                 uint32_t min_words, uint32_t max_gap, uint32_t min_works, uint32_t max_share,
                 uint32_t weight, uint32_t min_shared, uint32_t min_score,
                 fs_misquote_work* works, fs_misquote* misquotes, uint64_t cap_m,
                 uint64_t* n_misquotes, fs_misquote_pair* pairs, uint64_t cap_p,
                 uint64_t* n_pairs);
/* HIP-event milliseconds of the last fs_misquotes call on this thread: passages (with the
 * checks of the records), cells, number (classify and number the misquotes), postings, expand,
 * place (keep, partners, closest, the kept pairs in order), detail (with the copies out), and
 * the total of the seven; 0 for a pass that did not run.  tools/misquotes_bench.py.  There is
 * no _rows twin: fs_row carries no fan word (see fs_variants). */
int fs_misquotes_times(double* ms);

/* `ao3.py saturation`: what a sample of the fan works would show, the accumulation (rarefaction)
 * curve of the quoted units.  Records, passages, active works (numbered in work order), the
 * coverage, unit_of[n_script] and works(u), the active works quoting unit u, as for
 * fs_intervals.  n_works is every work of the file, active or not; a sample draws from all of
 * them.  A unit is quoted when works(u) > 0; Q is their number.  In order r (0-based, r <
 * permutations) work w (its work number) arrives at time h(r, w), the hash of fs_intervals with
 * r in place of the replicate,
 *     z = ((r << 32) | w) + seed * 0x9E3779B97F4A7C15                  (mod 2^64)
 *     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *     z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *     z =  z ^ (z >> 31);  h = z >> 32
 * a pure function of (seed, r, w).  Nothing is sorted or ranked: the sample at fraction f is the
 * works with h < f * 2^32, each work in it independently with probability f, and the samples
 * are nested as f grows.  Point c (1..points) has the threshold T_c = floor(c * 2^32 / points),
 * so T_points = 2^32, and
 *     bucket(h, points) = ((h + 1) * points + 2^32 - 1) >> 32          (64 bits)
 * is the first point whose sample holds a work of time h.
 *     first(r, u) = the smallest h(r, w) over the active works quoting u
 *     n_r(c)      = the works, of all n_works, with h(r, w) < T_c
 *     S_r(c)      = the quoted units with first(r, u) < T_c
 * so n_r(points) = n_works and S_r(points) = Q in every order.  Per point, with s the S_r(c) in
 * ascending order and t = permutations * (100 - level) / 200 (rounded down): low = s[t], high =
 * s[permutations - 1 - t], median = s[(permutations - 1) / 2], min = s[0], max =
 * s[permutations - 1] and the sum over r; the same three order statistics and the sum over the
 * n_r(c).  Per order: half_at, the smallest c with 2 * S_r(c) >= Q; ninety_at, with 10 * S_r(c)
 * >= 9 * Q; all_at, with S_r(c) == Q; all three 1 when Q = 0.  Every output is an integer. */
typedef struct fs_saturation_point {
  uint32_t units_low;        /* s[t] of S_r(c)                                            */
  uint32_t units_median;     /* s[(permutations - 1) / 2]                                 */
  uint32_t units_high;       /* s[permutations - 1 - t]                                   */
  uint32_t units_min;        /* s[0]                                                      */
  uint32_t units_max;        /* s[permutations - 1]                                       */
  uint32_t works_low;        /* the three order statistics of n_r(c)                      */
  uint32_t works_median;
  uint32_t works_high;
  uint64_t units_sum;        /* the sum of S_r(c) over r                                  */
  uint64_t works_sum;        /* the sum of n_r(c) over r                                  */
  uint64_t reserved0;        /* 0                                                         */
  uint64_t reserved1;        /* 0                                                         */
} fs_saturation_point;       /* 64 bytes                                                  */

typedef struct fs_saturation_perm {
  uint32_t half_at;          /* the smallest c with 2 * S_r(c) >= Q                       */
  uint32_t ninety_at;        /*                     10 * S_r(c) >= 9 * Q                  */
  uint32_t all_at;           /*                     S_r(c) == Q                           */
  uint32_t reserved;         /* 0                                                         */
} fs_saturation_perm;        /* 16 bytes                                                  */

typedef struct fs_saturation_summary {
  uint32_t n_active;         /* the works with a passage                                  */
  uint32_t units_quoted;     /* Q                                                         */
  uint32_t singletons;       /* Q1, the units with works(u) == 1                          */
  uint32_t doubletons;       /* Q2, the units with works(u) == 2                          */
} fs_saturation_summary;     /* 16 bytes                                                  */

#define FS_SATURATION_MAX_PERMUTATIONS 4096u
#define FS_SATURATION_MAX_POINTS 1024u
#define FS_SATURATION_MAX_WORKS (1u << 28)
/* Counted: the incidence matrix (ceil(n_units / 64) * 64 * ceil(active works / 64) * 8 bytes),
 * the first times (4 bytes per unit and order, the orders padded to a multiple of 64), the two
 * histograms (4 bytes per point and padded order, twice) and, where it is used, the table of
 * times (4 bytes per active work and padded order).  Their sum may be up to this. */
#define FS_SATURATION_MAX_BYTES (1u << 30)

/* Host columns and the host unit map in; works[n_units] (works(u)), pts[points] (pts[c - 1] is
 * point c), perms[permutations] and one summary out, on HIP device `device`; first is null or
 * [n_units][permutations], first(r, u) at first[u * permutations + r], 0xFFFFFFFF for a unit
 * nobody quotes (a quoted unit is recognised by works(u) > 0, never by that value: a time may be
 * 0xFFFFFFFF).  Both entry points: FS_E_INVALID for null arguments, min_words == 0, permutations
 * outside 1..FS_SATURATION_MAX_PERMUTATIONS, points outside 1..FS_SATURATION_MAX_POINTS, level
 * outside 50..99, records out of (work, fan_ix) order, a work >= n_works, an orig_ix >= n_script
 * or a unit_of entry that is neither below n_units nor 0xFFFFFFFF; FS_E_UNSUPPORTED for n_rows
 * >= 2^32, n_script > FS_WORKS_MAX_SCRIPT, n_works > FS_SATURATION_MAX_WORKS or tables above
 * FS_SATURATION_MAX_BYTES (the message states the parts).  No records, no active work and no
 * units follow the definitions: Q = 0, every S_r(c) is 0 and the three per-order figures are 1;
 * the n_r(c) count the works of the file all the same.
 * The passes are separate launches and no workgroup waits on another; every merge is an integer
 * min or add, so any schedule gives the same result: incidence (fs_companions' own) with
 * works(u) and the summary's counts; the sample sizes, a workgroup per order and slab of works
 * that hashes every work of the file into a histogram over the points in LDS and adds its
 * non-zero buckets, then a scan over c; the min product, a wave per unit row and 64 orders at
 * a time, a lane per order, the set bits of the row walked by wave-uniform control, one min per
 * set bit against the work's time; the curve, bucket(first) of the quoted units into histograms in LDS
 * per tile of units and 64 orders, added to hist[c][r], a scan over c, a lane per order for its
 * three figures; and per point a workgroup that sorts the S_r(c) and the n_r(c) in LDS.
 * Switches of the environment, read once per call; the output is the same wherever they stand:
 *   FS_SATURATION_TABLE      where the product takes a work's time from.  1: a table
 *                            time[active work][orders padded to 64], written once by a pass of
 *                            its own, a set bit then one coalesced 256-byte read per wave;
 *                            0 (default): the hash made again in the lane.  A call whose tables
 *                            would pass the byte limit with the table of times and not without
 *                            it takes 0
 *   FS_SATURATION_OSPLIT     the workgroups that share the chunks of 64 orders of a unit row;
 *                            a wave reads its row once for all the chunks it takes.  Default:
 *                            1 from 2048 workgroups of four rows on, more below, a chunk each at
 *                            the most
 *   FS_SATURATION_KSPLIT     the workgroups that share the words of a unit row and merge their
 *                            parts by an atomic min; default: 1 from 512 product workgroups on,
 *                            more below, at least 8 words each
 *   FS_SATURATION_MAX_BYTES  a lower bound than the macro's, for tests */
int fs_saturation(int device, const uint32_t* work, const uint32_t* fan_ix,
                  const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works, uint32_t n_script,
                  const uint32_t* unit_of, uint32_t n_units, uint32_t min_words, uint32_t max_gap,
                  uint32_t permutations, uint32_t points, uint64_t seed, uint32_t level,
                  uint32_t* works, fs_saturation_point* pts, fs_saturation_perm* perms,
                  fs_saturation_summary* summary, uint32_t* first);
/* The same over device-resident fs_row records (16-byte aligned) and a device-resident unit map
 * of the index's n_script entries into device buffers (d_points, d_perms and d_summary 16-byte
 * aligned, d_works and d_first 4-byte; d_first may be null), on the index's device and stream;
 * returns when they are written. */
int fs_saturation_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                       const uint32_t* d_unit_of, uint32_t n_units, uint32_t min_words,
                       uint32_t max_gap, uint32_t permutations, uint32_t points, uint64_t seed,
                       uint32_t level, uint32_t* d_works, fs_saturation_point* d_points,
                       fs_saturation_perm* d_perms, fs_saturation_summary* d_summary,
                       uint32_t* d_first);
/* Of the last fs_saturation / fs_saturation_rows call on this thread, ten doubles: HIP-event
 * milliseconds of incidence (with works(u) and the summary's counts), sample sizes (with their
 * scan), the table of times, the product, the curve (with its scan and the per-order figures),
 * the per-point statistics (with the copies out), and the total of the six; 0 for a pass that
 * did not run.  Then 1 when the product read the table of times and 0 when it hashed, the
 * shares of a unit row's words and the shares of its chunks of orders.
 * tools/saturation_bench.py. */
int fs_saturation_times(double* ms);
/* bucket(h, points) as the kernels compute it, points from 1 to FS_SATURATION_MAX_POINTS.  No
 * device is touched. */
uint32_t fs_saturation_bucket(uint32_t h, uint32_t points);

/* `ao3.py transitions`: which stretch of the script the fan works quote next, the directed
 * complement of fs_companions.  Records and passages as for fs_passages, in record order;
 * passage p has fan_first / fan_last and orig_first / orig_last as in fs_retelling_passage.
 * unit_of[n_script] as for fs_companions; the unit of a passage is unit_of[orig_first], and a
 * passage without a unit is left out: it neither counts nor breaks anything.
 *  - A work's sequence is its unit-bearing passages in record order, p_1 .. p_m.
 *  - A step is a pair (p_k, p_k+1) of the sequence with within == 0xFFFFFFFF (any distance) or
 *    fan_first(p_k+1) - fan_last(p_k) <= within + 1 (in 64 bits): at most `within` fan words
 *    lie between the two.  It goes from a = unit(p_k) to b = unit(p_k+1); a == b is a loop.  It
 *    advances when orig_first(p_k+1) > orig_last(p_k), the following rule of fs_retellings.
 *  - Cell (a, b): its steps, those that advance, the distinct works with such a step and the
 *    smallest of them.  steps_out(a) and steps_in(b) sum over all cells, kept or not.
 *  - A cell is kept when steps >= min_steps, works >= min_step_works and steps * 100 >=
 *    min_share * steps_out(a) (the product in 64 bits; min_share a whole percentage, 0..100;
 *    exactly at the bound is kept).
 * Every output is an integer: adds and minima commute, set membership does not depend on who
 * inserted, ties are settled by single 64-bit keys and places come from scanned counts, so no
 * schedule changes the result. */
typedef struct fs_transition_unit {
  uint32_t passages;         /* unit-bearing passages in the unit                       */
  uint32_t works;            /* distinct works with one                                 */
  uint32_t starts;           /* works whose sequence begins in the unit                 */
  uint32_t ends;             /* works whose sequence ends in it (one passage: both)     */
  uint32_t steps_out, steps_in;
  uint32_t successors;       /* kept cells (u, .)                                       */
  uint32_t predecessors;     /* kept cells (., u)                                       */
  uint32_t best_next;        /* the b of the kept cell (u, b) with the most steps, the
                                smaller b on a tie; 0xFFFFFFFF without a kept cell      */
  uint32_t best_steps;       /* its steps; 0 without one                                */
} fs_transition_unit;        /* 40 bytes                                                */

typedef struct fs_transition {
  uint32_t a, b;             /* from unit a to unit b                                   */
  uint32_t steps, advances;
  uint32_t works, first_work;
  uint32_t steps_out_a, steps_in_b;
} fs_transition;             /* 32 bytes                                                */

/* Host columns and the host unit map in; units[n_units] and `cap` cells out, on HIP device
 * `device`.  The kept cells come in (a, b) ascending order.  Both entry points: FS_E_INVALID for
 * null arguments, min_words, min_steps or min_step_works == 0, min_share > 100, records out of
 * (work, fan_ix) order, a work >= n_works, an orig_ix >= n_script or a unit_of entry that is
 * neither below n_units nor 0xFFFFFFFF; FS_E_UNSUPPORTED for n_rows >= 2^32 or n_script >
 * FS_WORKS_MAX_SCRIPT; FS_E_CAPACITY with *n_cells = cells required when cap is smaller (units
 * is complete then, cells untouched).  n_rows == 0 or n_units == 0: units of zeros with
 * best_next 0xFFFFFFFF, *n_cells = 0 (fs_transitions: without device work, the unit map unread).
 * Device memory is a few words per record and per unit.  Up to FS_TRANSITIONS_DENSE units
 * (default and most 64; 0: never) the cells are a plain n_units x n_units array that every
 * workgroup accumulates in LDS; beyond it they are the slots of a hash table.
 * FS_TRANSITIONS_HASH_BITS keeps that many bits of every hash (0: every key probes from slot
 * 0).  Both are diagnostics of the environment, read on each call; the output is the same
 * wherever they stand. */
int fs_transitions(int device, const uint32_t* work, const uint32_t* fan_ix,
                   const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works, uint32_t n_script,
                   const uint32_t* unit_of, uint32_t n_units, uint32_t min_words,
                   uint32_t max_gap, uint32_t within, uint32_t min_steps,
                   uint32_t min_step_works, uint32_t min_share, fs_transition_unit* units,
                   fs_transition* cells, uint64_t cap, uint64_t* n_cells);
/* The same over device-resident fs_row records (16-byte aligned) and a device-resident unit map
 * of the index's n_script entries into device buffers (4-byte aligned), on the index's device
 * and stream; returns when they are written. */
int fs_transitions_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                        const uint32_t* d_unit_of, uint32_t n_units, uint32_t min_words,
                        uint32_t max_gap, uint32_t within, uint32_t min_steps,
                        uint32_t min_step_works, uint32_t min_share,
                        fs_transition_unit* d_units, fs_transition* d_cells, uint64_t cap,
                        uint64_t* n_cells);
/* HIP-event milliseconds of the last fs_transitions / fs_transitions_rows call on this thread:
 * sequence (checks, run heads, the unit-bearing passages listed), count (the steps and every
 * figure behind them), keep (the keep rule, the scan, the per-unit results), place (scatter and
 * rank), and the total of the four; 0 for a pass that did not run.
 * tools/transitions_bench.py. */
int fs_transitions_times(double* ms);

/* `ao3.py sources`: which script each fan passage quotes, the join of K searches of one corpus
 * against K scripts.  File s (script s, 0-based) is the records of one search as columns sorted
 * by (work, fan_ix), the work numbers shared by all files; its passages are those of
 * fs_passages under the same min_words and max_gap.  Passage p has a script s(p), a work, the fan
 * span [fan_first, fan_last] and the script span [orig_first, orig_last] of its first and last
 * record; its span length is fan_last - fan_first + 1 in 64 bits.
 *  - q is a rival of p when s(q) != s(p), both are of one work, and q.fan_first <= p.fan_last
 *    and p.fan_first <= q.fan_last (one common word is enough; adjacent spans are no rivals).
 *    overlap(p, q) is the length of the intersection.
 *  - key(p) = (n_words, n_exact, -script), a total order across scripts.  p is alone
 *    (FS_SOURCE_ALONE) without a rival, won (FS_SOURCE_WON) when key(p) > key(q) for every rival
 *    q, lost (FS_SOURCE_LOST) otherwise: a local maximum, so a passage that loses to a passage
 *    which lost itself is still lost.
 *  - The best rival is the rival with the largest (n_words, n_exact, -script, -fan_first,
 *    -first).
 *  - contested_words is the number of fan words of p's span inside at least one rival's span (a
 *    union: a word two rivals cover counts once); sole_words is the span length less that.
 *  - A (work, script) row exists where the script has a passage in the work; primary is 1 for
 *    the script with the most covered_words (the sum of span lengths) in the work, the smaller
 *    script on a tie.
 *  - Pair (a, b), a < b: the rival pairs (p of a, q of b) are its contests, shared_words the sum
 *    of their overlaps, a_wins those with key(p) > key(q), b_wins the rest.  Two passages of one
 *    file that touch in a word (a file with two records at one fan index) both meet a rival
 *    that covers it: pair sums count that word twice, contested_words once.
 * Every value is an integer; adds and maxima commute, ties are settled by total orders and
 * places come from counts, so no schedule changes the result. */
#define FS_SOURCES_MAX_FILES 64u
#define FS_SOURCES_MAX_BYTES (1ull << 30)
#define FS_SOURCE_ALONE 0u
#define FS_SOURCE_WON 1u
#define FS_SOURCE_LOST 2u

typedef struct fs_source_cols {
  const uint32_t* work;      /* [n] each, sorted by (work, fan_ix)                        */
  const uint32_t* fan_ix;
  const uint32_t* orig_ix;
  const double* comb;
  uint64_t n;
} fs_source_cols;            /* 40 bytes                                                  */

typedef struct fs_source_passage {
  uint32_t script, work;
  uint32_t first;            /* index of its first record in its file's columns           */
  uint32_t n_words, n_exact; /* as in fs_passage                                          */
  uint32_t fan_first, fan_last, orig_first, orig_last;
  uint32_t rivals;           /* rival passages                                            */
  uint32_t rival_scripts;    /* distinct scripts among them                               */
  uint32_t outcome;          /* FS_SOURCE_ALONE / _WON / _LOST                            */
  uint32_t best_rival;       /* its script; 0xFFFFFFFF when alone                         */
  uint32_t best_rival_words; /* its n_words and fan_first; 0 when alone                   */
  uint32_t best_rival_fan_first;
  uint32_t reserved;         /* 0                                                         */
  uint64_t contested_words, sole_words;
} fs_source_passage;         /* 80 bytes                                                  */

typedef struct fs_source_work {
  uint32_t work, script;
  uint32_t passages, alone, won, lost;
  uint32_t work_scripts;     /* scripts with a passage in this work                       */
  uint32_t primary;          /* 1: the script with the most covered_words in the work     */
  uint64_t covered_words, contested_words, sole_words;
} fs_source_work;            /* 56 bytes                                                  */

typedef struct fs_source_script {
  uint32_t works, passages, alone, won, lost, primary_works;
  uint64_t covered_words, contested_words, sole_words;
} fs_source_script;          /* 48 bytes                                                  */

typedef struct fs_source_pair {
  uint32_t a, b;             /* a < b                                                     */
  uint32_t works_both;       /* works with a passage of each                              */
  uint32_t reserved;         /* 0                                                         */
  uint64_t contests, shared_words, a_wins, b_wins;
} fs_source_pair;            /* 48 bytes                                                  */

/* Host columns of n_files files in; out, on HIP device `device`: the passages of all files in
 * (work, fan_first, script, first) order, the (work, script) rows in (work, script) order,
 * scripts[n_files] and pairs[n_files (n_files - 1) / 2] in (a, b) order ((0, 1), (0, 2) ...).
 * FS_E_INVALID for null arguments, n_files == 0, min_words == 0, records out of (work, fan_ix)
 * order or a work >= n_works; FS_E_UNSUPPORTED, before anything is read, for n_files >
 * FS_SOURCES_MAX_FILES or a file of 2^32 records or more, and for device memory above
 * FS_SOURCES_MAX_BYTES, which counts 28 bytes per record of the largest file and 12 per work
 * (refused before anything is read), then 160 bytes per passage and 56 per (work, script) row.
 * FS_E_CAPACITY with *n_passages and *n_work_rows = the counts required when either cap is
 * smaller: scripts and pairs are complete then, passages and works untouched.  Files are read
 * one after the other; a file without records has no passages.
 * Diagnostics of the environment, read on each call; the output is the same wherever they
 * stand:
 *   FS_SOURCES_PACK   1 (default): a wave takes 64 / K2 passages in the contest pass, K2 the
 *                     power of two at or above n_files; 0: one passage per wave
 *   FS_SOURCES_UNION  0 (default): contested_words of a passage with rivals of one script is
 *                     that script's overlaps, only passages with rivals of two or more scripts
 *                     take the union pass; 1: every contested passage takes it
 *   FS_SOURCES_DENSE  n_files up to which a workgroup of the contest pass keeps the pair
 *                     figures in LDS (default and most 64; 0: every figure a global atomic) */
int fs_sources(int device, const fs_source_cols* files, uint32_t n_files, uint32_t n_works,
               uint32_t min_words, uint32_t max_gap, fs_source_passage* passages,
               uint64_t cap_passages, uint64_t* n_passages, fs_source_work* works,
               uint64_t cap_works, uint64_t* n_work_rows, fs_source_script* scripts,
               fs_source_pair* pairs);
/* HIP-event milliseconds of the last fs_sources call on this thread: passages (every file's
 * uploads, checks, run heads and passage columns), contest (rivals, outcomes, places, pair
 * figures), union (contested words of the passages that need the union pass), rollups (rows,
 * scripts, pairs), and the total of the four; 0 for a pass that did not run.
 * tools/sources_bench.py. */
int fs_sources_times(double* ms);

/* `ao3.py alignments`: quotes with inserted or dropped words, a gapped local alignment of every
 * fan work against the script.  Records sorted by (work, fan_ix) as for fs_passages (comb: their
 * BEST_COMBINED_DISTANCE).  With R = reach, S = match, P = gap, all integers:
 *  - For records j < i of one work let df = fan_ix(i) - fan_ix(j) and do = orig_ix(i) -
 *    orig_ix(j), signed.  j may precede i when 1 <= df <= R + 1 and 1 <= do <= R + 1; the link
 *    costs P * ((df - 1) + (do - 1)).  j need not be i - 1: records between them are skipped.
 *  - best(i) = S + max(0, max over the j that may precede i of best(j) - cost(j, i)).
 *  - prev(i) is the j at that maximum when it is above 0, the largest j (the nearest record) on
 *    a tie; otherwise i is a root.  root(i) = root(prev(i)), or i for a root.
 *  - The records of one root are a tree.  Its peak is its record with the largest best, the
 *    smallest index on a tie; its alignment is the path from the root to the peak along prev.
 *    The tree's other records are side records: counted, not reported as alignments.
 *  - An alignment is kept when its path has at least min_words records; the kept alignments are
 *    listed in root order, that is by (work, first fan word).
 * Every output is an integer below 2^32; candidates are compared as (value, j) and peaks as
 * (best, ~i), total orders: no schedule changes the result.  At reach 0 every link costs 0, and
 * on records without two at one fan index the kept alignments are the passages of fs_passages
 * at max_gap 0. */
typedef struct fs_alignment {
  uint64_t first, last;                /* record index of the root and of the peak                */
  uint32_t n_words, n_exact;           /* path records; those with comb <= 0 (NaN never counts)   */
  uint32_t score;                      /* best(peak)                                              */
  uint32_t fan_skipped, orig_skipped;  /* sums of df - 1 and of do - 1 along the path             */
  uint32_t pieces;                     /* 1 + the links with df != 1 or do != 1                   */
  uint32_t tree_records;               /* records of the whole tree, side records included        */
  uint32_t reserved;                   /* 0                                                       */
  uint64_t path_at;                    /* offset of the path's records in `path`                  */
} fs_alignment;                        /* 56 bytes (two 8-byte indices, eight words, one offset)  */

/* Host columns in; `cap` alignments and `path_cap` path records out, on HIP device `device`:
 * path holds the record indices of every kept alignment, path after path, each in path order.
 * Both entry points: FS_E_INVALID for null arguments, min_words == 0, match == 0, reach > 63,
 * match or gap above 16, or records out of (work, fan_ix) order; FS_E_UNSUPPORTED for n_rows >=
 * 2^32 or n_rows * match >= 2^32; FS_E_CAPACITY with *n_out = alignments and *n_path = path
 * records required when either buffer is too small (both untouched then).  n_rows == 0: FS_OK
 * with both counts 0, without device work.  Device memory is a dozen words per record.
 * A record starts a segment when its work changes or its fan index is more than R + 1 past the
 * record in front of it; no link crosses that.  Segments of up to FS_ALIGNMENTS_SMALL records
 * (default 8; 0: none) take a lane each, longer ones a wave each with the last 64 records in
 * registers; candidates behind those 64 (records sharing a fan index) are read back from
 * global memory, and with FS_ALIGNMENTS_RING=0 every candidate is.  Both are diagnostics of
 * the environment, read on each call; the output is the same wherever they stand. */
int fs_alignments(int device, const uint32_t* work, const uint32_t* fan_ix,
                  const uint32_t* orig_ix, const double* comb, uint64_t n_rows,
                  uint32_t min_words, uint32_t reach, uint32_t match, uint32_t gap,
                  fs_alignment* out, uint64_t cap, uint64_t* n_out, uint32_t* path,
                  uint64_t path_cap, uint64_t* n_path);
/* The same over device-resident fs_row records (16-byte aligned) into device buffers (d_out
 * 8-byte, d_path 4-byte aligned), on the index's device and stream; returns when they are
 * written. */
int fs_alignments_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t min_words,
                       uint32_t reach, uint32_t match, uint32_t gap, fs_alignment* d_out,
                       uint64_t cap, uint64_t* n_out, uint32_t* d_path, uint64_t path_cap,
                       uint64_t* n_path);
/* HIP-event milliseconds of the last fs_alignments / fs_alignments_rows call on this thread:
 * segments (order check, heads), bins (the segments by class), chain (the recurrence, both
 * classes), keep (kept roots, their places, the alignment records), trace (the path records),
 * and the total of the five; 0 for a pass that did not run.  tools/alignments_bench.py. */
int fs_alignments_times(double* ms);

/* `ao3.py matrix --engine device`: the n-grams behind the works x phrases matrix.  Records
 * sorted by (work, fan_ix), in the order the command takes them (works by first appearance,
 * stable by fan index).
 *  - A fan run starts where the work changes or fan_ix is not the previous record's + 1
 *    (compared without 32-bit wrap): a repeated fan index splits a run.
 *  - Inside a fan run, c(v) is the number of records that name script word v.  The distinct v
 *    are walked in ascending order with an open interval: v extends the interval when it ends
 *    at v - 1, else the interval is closed and [v, v] opened; then, if c(v) >= 2, the interval
 *    is closed at v, c(v) - 2 single-word spans [v, v] follow, and [v, v] is opened again.
 *    The closed intervals of at least `ngram` words are the spans.
 *  - starts[s] is the number of spans [a, b] with a <= s <= b - ngram + 1, over all works.
 *  - A span's n-gram starts at the first s in a .. b - ngram + 1 with the largest starts[s].  It
 *    is kept iff starts[s'] < starts[s] for every s' in [s - ngram + 1, s) and starts[s'] <=
 *    starts[s] for every s' in (s, s + ngram); positions below 0 or from n_script on count 0.
 *  - out is the kept n-grams in span order: works, then fan runs in record order, then spans
 *    by ascending first word (equal spans give equal n-grams).
 * Every value is an integer: no schedule changes a result. */
typedef struct fs_matrix_ngram {
  uint32_t work, start;
} fs_matrix_ngram;                     /* 8 bytes                                                 */

/* Device memory of a call, counted before anything runs: 20 bytes for every slot of the table
 * of c(v) (the power of two that is at least twice n_rows, and at least 64), 40 bytes a record
 * (the lists of runs and spans at their largest) and 8 bytes a script word. */
#define FS_MATRIX_MAX_BYTES (1u << 30)

/* Host columns in; starts[n_script] (or null) and `cap` n-grams out, on HIP device `device`.
 * Both entry points: FS_E_INVALID for null arguments, ngram == 0, records out of (work, fan_ix)
 * order, a work >= n_works or a script index >= n_script; FS_E_UNSUPPORTED for n_rows >= 2^32,
 * n_script > FS_WORKS_MAX_SCRIPT or tables above FS_MATRIX_MAX_BYTES; FS_E_CAPACITY with
 * *n_kept = n-grams required when cap is smaller (starts and *n_spans are complete then, out
 * untouched); n_rows / ngram + 1 always suffices.  *n_spans: the spans of at least ngram words.
 * n_rows == 0: zeros, without device work in fs_matrix.  A span of up to FS_MATRIX_SMALL
 * (default 32) starts is handled by a lane, a longer one by a wave; FS_MATRIX_HASH_BITS keeps
 * that many bits of the hash behind the table of c(v) (0: every key collides).  Both are
 * diagnostics of the environment, read on each call; the output is the same wherever they
 * stand. */
int fs_matrix(int device, const uint32_t* work, const uint32_t* fan_ix, const uint32_t* orig_ix,
              uint64_t n_rows, uint32_t n_works, uint32_t n_script, uint32_t ngram,
              uint32_t* starts, fs_matrix_ngram* out, uint64_t cap, uint64_t* n_spans,
              uint64_t* n_kept);
/* The same over device-resident fs_row records (16-byte aligned) into device buffers (4-byte
 * aligned; d_starts may be null), on the index's device and stream; returns when they are
 * written. */
int fs_matrix_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                   uint32_t n_script, uint32_t ngram, uint32_t* d_starts, fs_matrix_ngram* d_out,
                   uint64_t cap, uint64_t* n_spans, uint64_t* n_kept);
/* HIP-event milliseconds of the last fs_matrix / fs_matrix_rows call on this thread: runs
 * (checks, run heads, the table of c(v)), spans (span ends, spans per run, the difference
 * array), counter (its running sum), pick (the span list, places, n-grams and their
 * neighbourhoods), place (the kept n-grams counted and written), and the total of the five; 0
 * for a pass that did not run.  tools/matrix_bench.py. */
int fs_matrix_times(double* ms);

/* ---- `ao3.py passages / works / quotes`: the match CSV read on the device ----
 * The twelve-column file `search` writes (csv.writer's defaults, distances by repr), with its
 * header row or without: the bytes in, the non-empty rows out as a field index, the numeric
 * columns fs_passages / fs_works / fs_quotes take, and a head flag per row.  The reader does not
 * guess.  A '"' toggles quoting, ',' outside quotes ends a field, '\n' outside quotes ends a row
 * (a '\r' directly in front belongs to the terminator, a last row needs none); this equals
 * csv.reader when every opening quote starts a field, every closing quote is followed by ',',
 * a terminator, the end of the file or the second quote of a "" pair, no '\r' stands outside
 * quotes without its '\n', no NUL occurs and every non-empty row has twelve fields.  fan_ix,
 * orig_ix and lev are unquoted runs of 1..10 digits below 2^32.  A file that breaks any of this,
 * or is not UTF-8, is FS_MATCHES_OUTSIDE (info.reason: FS_MATCH_BAD_* bits) and nothing of it is
 * returned.  dist and comb: the empty field (NaN), nan, inf, -inf or a decimal of repr's shape
 * with up to 17 significant digits, converted to the bits float() gives; a field of another
 * shape is listed as deferred {row, column}, holds NaN, and is the host's to convert
 * (FS_MATCHES_DEFERRED; more than max(4096, n_rows / 16) of them: FS_MATCHES_OUTSIDE). */
#define FS_MATCH_FIELDS 12
enum { FS_MATCHES_PARSED = 0, FS_MATCHES_DEFERRED = 1, FS_MATCHES_OUTSIDE = 2 };
enum {
  FS_MATCH_BAD_NUL = 1,     /* a NUL byte                                               */
  FS_MATCH_BAD_OPEN = 2,    /* an opening quote inside a field                          */
  FS_MATCH_BAD_CLOSE = 4,   /* text behind a closing quote, or the file ends in quotes  */
  FS_MATCH_BAD_CR = 8,      /* '\r' outside quotes without '\n'                         */
  FS_MATCH_BAD_FIELDS = 16, /* a row without twelve fields                              */
  FS_MATCH_BAD_INT = 32,    /* fan_ix, orig_ix or lev is not 1..10 plain digits < 2^32  */
  FS_MATCH_BAD_UTF8 = 64,   /* malformed UTF-8                                          */
  FS_MATCH_BAD_ROW = 128,   /* a row of 2^32 bytes or more                              */
  FS_MATCH_BAD_DEFER = 256  /* too many numeric fields left to the host                 */
};

/* Where the fields of row r lie: field f is bytes[start + (f ? end[f - 1] + 1 : 0) ..
 * start + end[f]), for a quoted field (bit f of `quoted`) with its quotes, "" pairs as
 * written.  head: FAN_WORK_FILENAME's bytes differ from those of the row in front (1 for the
 * first row); equal names written differently both count as heads, the host merges them. */
typedef struct fs_match_ix {
  uint64_t start;                /* offset of the row's first byte in the file           */
  uint32_t end[FS_MATCH_FIELDS]; /* end of every field, relative to start                */
  uint32_t quoted;
  uint32_t head;
} fs_match_ix;                   /* 64 bytes                                             */

typedef struct fs_match_defer {
  uint32_t row, col;             /* col: 9 BEST_MATCH_DISTANCE, 11 BEST_COMBINED_DISTANCE */
} fs_match_defer;

typedef struct fs_matches_info {
  uint64_t n_rows;       /* non-empty rows, the header row not counted                   */
  uint64_t n_deferred;
  uint32_t status;       /* FS_MATCHES_*                                                 */
  uint32_t reason;       /* FS_MATCH_BAD_* bits when outside                             */
  uint32_t has_header;   /* the first non-empty row is the header row, byte for byte     */
  uint32_t reserved;
  double   ms[8];        /* HIP-event times: upload, quote parity + scan, classify, row scan
                            + placement, header look + buffers, rows, all of them, 0     */
} fs_matches_info;       /* 96 bytes                                                     */

/* The file's bytes (host memory) read on HIP device `device`; the handle keeps the bytes and
 * the results on the device until fs_matches_close.  An empty file or the header alone: zero
 * rows, no device work.  FS_E_UNSUPPORTED for 2^32 rows or more.  A handle is returned for an
 * outside file too (only its info is of use). */
typedef struct fs_matches fs_matches;
int fs_matches_open(int device, const uint8_t* bytes, uint64_t n_bytes, fs_matches** out,
                    fs_matches_info* info);
/* The columns and the index of the info.n_rows rows and the deferred fields (in no order) into
 * host buffers of `cap` rows and `defer_cap` entries; FS_E_CAPACITY when either is too small
 * (the info says what is needed), FS_E_INVALID for an outside file. */
int fs_matches_read(fs_matches* m, uint32_t* fan_ix, uint32_t* orig_ix, uint32_t* lev,
                    double* dist, double* comb, fs_match_ix* ix, uint64_t cap,
                    fs_match_defer* deferred, uint64_t defer_cap);
/* The label check of `works` and `quotes`: first[w] = smallest row whose orig_ix is w
 * (0xFFFFFFFF: none), *n_differ = rows whose field `column` differs in its bytes from that of
 * first[their orig_ix].  0: the column is a function of the script word and first[] names one
 * row to decode per word; otherwise two spellings occur (two labels, or one quoted two ways)
 * and the host decides.  FS_E_INVALID for an orig_ix >= n_script or column >= 12. */
int fs_matches_labels(fs_matches* m, uint32_t column, uint32_t n_script, uint32_t* first,
                      uint64_t* n_differ);
/* The distinct spellings of text column `column`, numbered on the device (`ao3.py variants`):
 * id[info.n_rows], and the first row of every spelling into first[cap].  Two rows get the same
 * id exactly when the bytes of the field are equal, quotes and "" pairs as written (bytes are
 * compared, never hashes alone); a field quoted in one row and bare in another is two
 * spellings, and the host merges the spellings that decode to the same text.  Ids are in
 * first-appearance order: id[r] = the distinct spellings whose first row lies before the first
 * row of r's spelling, what ids.setdefault(text, len(ids)) gives over the rows in file order;
 * first[k] = the smallest row with spelling k, ascending in k.  FS_E_CAPACITY with *n_distinct =
 * spellings when cap is smaller (id is complete then, first untouched); FS_E_INVALID for
 * column >= 12 or an outside file.  Zero rows: *n_distinct = 0, no device work.  The table and
 * the ids stay behind the handle until fs_matches_close.  FS_INTERN_HASH_BITS=k in the
 * environment (read per call; diagnostic) keeps k bits of the hash, 0: every string collides. */
int fs_matches_intern(fs_matches* m, uint32_t column, uint32_t* id, uint32_t* first,
                      uint64_t cap, uint64_t* n_distinct);
/* HIP-event times of the handle's last fs_matches_intern into ms[8]: clearing the table,
 * insert, numbering (count, scan, number, ids), copies out, all of them, 0, 0, 0. */
int fs_matches_intern_times(const fs_matches* m, double* ms);
void fs_matches_close(fs_matches* m);
/* The conversion the reader applies to dist and comb, on the host (no GPU involved): 0 and
 * *out = float(text) bit for bit, or 1 ("not mine": *out untouched) as described above. */
int fs_matches_parse_double(const uint8_t* bytes, uint64_t len, double* out);

/* Timing events ride on every `period`-th scan launch only (default 1 = every
 * launch); searches in between report scan_ms = 0.  The events cost a few
 * microseconds of stream time per launch, which matters for sub-100 us searches. */
int fs_index_set_scan_timing(fs_index* ix, uint32_t period);

/* Diagnostics: name of the kernel that dominates a search of `c` on `ix` as things stand
 * (pipeline, window size, corpus size, switches), e.g. "k_scan_rows<6,4>": what a profile
 * of the search lists first.  Static storage, valid until the next call on this thread. */
const char* fs_search_kernel_name(fs_index* ix, fs_corpus* c);

/* Diagnostics: what a search of `c` on `ix` would launch as things stand (script length,
 * corpus size, lanes, switches), answered by the functions the launch itself asks.  The
 * index build and the launch choose buffer sizes, kernel instances, launch shapes and the
 * record form by the script's length; a test pins each choice at the length where it flips.
 * Read-only: nothing is queued or built (a view that has not been searched yet has no
 * batch table and reports the chained kernels). */
typedef struct fs_scan_shape {
  uint32_t waves;              /* waves per workgroup of k_scan_rows; 0: the chained kernels   */
  uint32_t blocks;             /* its workgroups; 0 with the chained kernels                   */
  uint32_t filter_log2_words;  /* log2 words of the filter k_scan_rows holds in LDS (the
                                  sub-shingle filter where it applies); with the chained
                                  kernels, of their Bloom filter                               */
  uint32_t seeds_lds_bytes;    /* displacement seeds k_scan_rows holds in LDS; 0: it reads
                                  them from memory (or the chained kernels run)                */
  uint32_t log2_buckets;       /* of the exact table's displacement seeds                      */
  uint32_t log2_slots;         /* of the exact table                                           */
  uint32_t overflow_buckets;   /* buckets placed by linear probing (n-grams with colliding
                                  32-bit hashes)                                               */
  uint32_t wide_buckets;       /* separable buckets whose seed does not fit a byte             */
  uint32_t host_wire8;         /* 1: an FS_ROWS_HOST search brings 8-byte wire records over
                                  and expands them on the host (exact pipeline, scripts below
                                  2^18 tokens); 0: it does not                                 */
  uint32_t ids16;              /* 1: k_scan_rows streams the corpus' 16-bit copy of the ids
                                  (every vector id of the batch below 2^16, no string ids of its
                                  own, FS_SCAN_IDS16 not 0), two pairs of sub-tiles in flight
                                  per wave; 0: the 32-bit ids                                  */
  uint32_t reserved[2];        /* 0                                                            */
} fs_scan_shape;               /* 48 bytes                                                     */
int fs_index_scan_shape(fs_index* ix, fs_corpus* c, fs_scan_shape* out);

/* ---- host text front end (search.py:164-166: read a fan work, tokenise, drop whitespace) ----
 * spaCy's tokenizer splits a text on whitespace and treats every chunk by itself, with a cache
 * chunk -> tokens; fs_textenc is that cache and the splitting, natively and on `threads` host
 * threads: files in, string ids out.  The host teaches it what a chunk's tokens are
 * (fs_textenc_add: the vocabulary's plain words to start with, then every chunk its rule
 * tokenizer has been run on); a chunk it has not been taught comes back as a placeholder
 * 0x80000000 | k with its text (unk_bytes[unk_off[k] .. unk_off[k+1])), never as a guess.
 * status[i]: 0 encoded; 1 left to the host (a text of 100000 bytes or more -- the reference
 * cuts such texts into pieces first, search.py:47-63 -- or malformed UTF-8); < 0: -errno of
 * the read.  The result pointers are the encoder's own buffers, valid until the next call on
 * it.  No GPU is involved. */
typedef struct fs_textenc fs_textenc;
int fs_textenc_create(fs_textenc** out);
void fs_textenc_destroy(fs_textenc* enc);
int fs_textenc_add(fs_textenc* enc, const uint8_t* chunk_bytes, const uint64_t* chunk_off, uint64_t n_chunks,
                   const uint64_t* piece_off, const uint32_t* piece_ids);
int fs_textenc_encode_files(fs_textenc* enc, const char* paths /* n_files strings, each 0-terminated */,
                            uint64_t n_files, uint32_t threads,
                            const uint32_t** tok, uint64_t* n_tok, const uint64_t** work_off /* n_files + 1 */,
                            const int32_t** status, const uint8_t** unk_bytes, const uint64_t** unk_off,
                            uint64_t* n_unk);
/* The same with the pass the search makes over a batch's tokens next (search.py:65-84 looks
 * every token's vector up; here a token's vector id is vec_of_sid[string id], n_sid entries):
 * tok_vec[i] = vector id of token i (0 for a placeholder), *n_oov = tokens whose vector id has
 * FS_OOV_FLAG set, *ids_equal = 1 when every token's vector id equals its string id (a batch
 * without capitalised or out-of-vocabulary words: no string ids need to travel to the GPU).
 * Made by the threads that encode, each for its own files.  FS_E_INVALID when a string id the
 * encoder was taught lies beyond n_sid. */
int fs_textenc_encode_files_vec(fs_textenc* enc, const char* paths, uint64_t n_files, uint32_t threads,
                                const uint32_t* vec_of_sid, uint64_t n_sid,
                                const uint32_t** tok, uint64_t* n_tok, const uint64_t** work_off,
                                const int32_t** status, const uint8_t** unk_bytes, const uint64_t** unk_off,
                                uint64_t* n_unk, const uint32_t** tok_vec, uint64_t* n_oov, int32_t* ids_equal);

/* Diagnostics: tables with near-synonyms -- the sizes of the connected components of the graph
 * of "near" vector pairs that the integer prefilters of the LSH pipeline work over (0 entries:
 * the graph was not built: the exact pipeline, or a proof that fails by one slot only).
 * *in_use = 1 when the prefilters run over component ids, 0 when the components were judged
 * too coarse (one holds an eighth of the table) and searches take the plain LSH pipeline.  On an
 * index that uses the share rule (fs_index_share_info) the components are those of its angular
 * relation, and *in_use = 1. */
int fs_index_component_sizes(const fs_index* ix, uint32_t* sizes, uint64_t cap, uint64_t* n,
                             uint32_t* in_use);

/* Diagnostics: the share rule of the LSH pipeline (tables whose vectors are not unit length, where
 * neither integer prefilter applies).  *flags = 0: not in use; else bit 0 the
 * windows' gate, bit 1 the pairs' test, bit 2 the gate over heavy subsets of both sides, bit 3
 * out-of-vocabulary fan tokens count as possibly near, bit 4 set.  *components / *largest: the
 * components of the relation "cosine > *gamma" over the table. */
int fs_index_share_info(const fs_index* ix, uint32_t* flags, uint32_t* components, uint32_t* largest,
                        double* gamma);

/* Diagnostics: with FS_SHARE_COUNT=1 in the environment when the index is built, k_share_scan counts
 * what passes what; this reads the eight counters and sets them to zero: windows, windows with a
 * key in the filter, (window, key) entries of the map, (window, script window) pairs through the
 * pairs' test, pairs whose distance was computed, windows flagged, windows flagged as they are (no
 * constraint, or no room), 0.  All zero when the counters are off or the rule is not in use. */
int fs_index_share_counts(fs_index* ix, uint64_t* out8);

/* Diagnostics: with FS_LSH_COUNT=1 in the environment when the index is built, the kernels that read
 * the one-slot maps count the windows by the branch they took; this reads the FS_LSH_COUNTERS
 * counters into out[] and sets them to zero.  Second stage of k_lsh_sift / k_lsh_sift2, a window in
 * one of these at most: [0] has the ids of a script n-gram and took that n-gram's record (its kept
 * matches, the n-gram itself among them), [1] has them and the n-gram keeps no match; ended by the exact one-slot map with [2] no, [3] one, [4] two script n-grams one
 * slot away; kept pending [5] by a distance within the threshold, [6] by more than two such
 * n-grams, [7] by a full bucket (asked first).  k_lsh_enum: [8]..[11] windows listed with one to
 * four n-grams within the threshold, [12] listed after the sort exchanged two of them, [13] listed
 * with the list cut at nearest_n (entries of the kept occurrences: the index keeps an n-gram's first
 * nearest_n); [14] / [15] windows that read one / two buckets of a chain behind
 * a full one and found its end; windows given up to the bucket walk [16] by a fifth n-gram, [17] by
 * a chain still full at its third bucket, [18] by two n-grams at the same distance (a window
 * counts under every reason it has).  The rest 0; all 0 when the counters are off. */
#define FS_LSH_COUNTERS 24
int fs_index_lsh_counts(fs_index* ix, uint64_t* out);

/* Diagnostics: one synchronous search of `c` (arguments as fs_search_corpus) with a HIP event
 * behind every kernel of it.  names: the kernels' names in launch order, '\n'-separated;
 * ms[i]: time from the previous mark to the one behind kernel i (its duration when nothing else
 * runs on the GPU); *n = number of entries (also when the buffers hold fewer).  What bench.py
 * names as the dominant kernel of a search that is more than one launch comes from here.
 * Not part of the search path. */
int fs_search_profile(fs_index* ix, fs_corpus* c, fs_row* rows, uint64_t cap, int rows_on_device,
                      char* names, uint64_t names_cap, double* ms, uint32_t ms_cap, uint32_t* n);

/* Diagnostics: the FS_* environment switches (kernel variants, forced capacities) are
 * read once at fs_index_create; a test or sweep that changes them on a live index
 * calls this to have them read again.  Not part of the search path. */
int fs_index_reload_switches(fs_index* ix);

/* Diagnostics: `reps` back-to-back launches of the scan kernel alone over `c`,
 * timed with one pair of HIP events; *avg_ms = time per launch.  Used by
 * tools/scan_sweep.py to compare kernel variants without per-launch event
 * overhead.  Not part of the search path. */
int fs_scan_benchmark(fs_index* ix, fs_corpus* c, uint32_t reps, double* avg_ms);

/* Diagnostics: the floor under k_scan_rows.  `reps` launches of a kernel that only READS the ids
 * of `c` in k_scan_rows' launch shape (a workgroup of sixteen waves per CU, contiguous runs of
 * 512-token sub-tiles, 16-byte loads, pairs requested ahead) and keeps nothing; *avg_ms = its
 * dispatch-to-completion time, HIP events on every dispatch, one launch at a time.  What a
 * search's own kernel takes above this is its own work. */
int fs_stream_floor(fs_index* ix, fs_corpus* c, uint32_t reps, double* avg_ms);

/* ---- the batch files (search.py:192-218 the twelve fields of a record, :331-334 write_records) ----
 * fs_row records in, the bytes csv.writer(out).writerows(records) puts into a batch file out:
 * FAN_WORK_FILENAME = name of rows[i].work, FAN_WORK_WORD / _ORTH_ID = text and spaCy key
 * (MurmurHash64A of the UTF-8 bytes, seed 1) of string fan_sid[i] of the strings added so far,
 * the ORIGINAL_SCRIPT_* columns = entry rows[i].orig_ix of the four tables of fs_csvw_set_script
 * (each the text a record shows: the lower-case word, its key in decimal, the character name,
 * the scene number; None = the empty string), distances by Python's repr(float).  `excel`
 * dialect: "\r\n" behind a record, a field quoted -- its quotes doubled -- when it holds ',',
 * '"', CR or LF.  A string table is {bytes, off[n + 1]}.  *out is the writer's own buffer, valid
 * until its next call; writing it to a file is the caller's.  No GPU is involved. */
typedef struct fs_csvw fs_csvw;
int fs_csvw_create(fs_csvw** out);
void fs_csvw_destroy(fs_csvw* w);
int fs_csvw_set_script(fs_csvw* w, uint64_t n_script,
                       const uint8_t* word_bytes, const uint64_t* word_off,
                       const uint8_t* orth_bytes, const uint64_t* orth_off,
                       const uint8_t* char_bytes, const uint64_t* char_off,
                       const uint8_t* scene_bytes, const uint64_t* scene_off);
int fs_csvw_add_strings(fs_csvw* w, const uint8_t* bytes, const uint64_t* off, uint64_t n);   /* ids go on counting */
uint64_t fs_csvw_strings(const fs_csvw* w);                                                  /* strings added so far */
int fs_csvw_format(fs_csvw* w, const fs_row* rows, uint64_t n_rows,
                   const uint8_t* name_bytes, const uint64_t* name_off, uint64_t n_works,
                   const uint32_t* fan_sid, const uint8_t** out, uint64_t* out_len);

/* `ao3.py fanon`: the phrases fan works share with each other and the script lacks.  The one
 * command that reads the corpus itself and no match records.  The fan tokens are dense ids
 * below n_ids, tok[work_off[w] .. work_off[w + 1]) those of work w; the scripts are ids of the
 * same numbering, canon[canon_off[s] .. canon_off[s + 1]) those of script s, FS_FANON_NO_ID for a
 * word no fan token equals.  With K = k:
 *  - Position p of a work of L tokens has a gram when p + K <= L: its K ids from p on.  A gram
 *    never spans two works.  occurrences(g) = positions holding g, works(g) = different works
 *    with one, first(g) = the smallest (work, p).
 *  - g is canon when its K ids stand consecutively inside one script; common when works(g) * 100
 *    > max_share * n_works (64-bit; n_works counts empty works too); shared when works(g) >=
 *    min_works and it is neither.  Canon and common do not exclude each other.
 *  - A passage is a maximal run of positions p..q of one work that all hold shared grams: tokens
 *    p .. q + K - 1, n_tokens = q - p + K; least and most = the smallest and largest works(g)
 *    of its grams.  Two passages are one phrase when their id sequences are equal, compared id
 *    by id; a phrase's first is the smallest (work, p) of its passages.
 *  - shared_tokens (canon_tokens) of a work = its tokens inside the gram of at least one shared
 *    (canon) position: a union, overlapping grams count a token once.
 * Every output is an integer; grams are told apart by comparing ids, never by hash alone. */
typedef struct fs_fanon_work {
  uint32_t n_tokens, n_positions;      /* positions: those with a gram                       */
  uint32_t shared_positions, canon_positions, common_positions;
  uint32_t n_passages;
  uint32_t shared_tokens, canon_tokens;
  uint32_t longest_start;              /* its longest passage, the first among equals: token */
  uint32_t longest_tokens;             /* index in the work and n_tokens; 0, 0 without one   */
} fs_fanon_work;                       /* 40 bytes                                           */

typedef struct fs_fanon_gram {
  uint32_t work, start;                /* first(g): work and token index in it               */
  uint32_t works, occurrences;
} fs_fanon_gram;                       /* 16 bytes                                           */

typedef struct fs_fanon_passage {
  uint32_t work, start, n_tokens;      /* start: token index in the work                     */
  uint32_t phrase;                     /* index into the phrases                             */
  uint32_t least, most;
} fs_fanon_passage;                    /* 24 bytes                                           */

typedef struct fs_fanon_phrase {
  uint32_t work, start;                /* first: work and token index in it                  */
  uint32_t n_tokens, n_passages, n_works;
  uint32_t least, most;
  uint32_t reserved;                   /* 0                                                  */
} fs_fanon_phrase;                     /* 32 bytes                                           */

#define FS_FANON_NO_ID 0xFFFFFFFFu     /* a script word that is no fan token                 */
#define FS_FANON_MIN_LENGTH 2u
#define FS_FANON_MAX_LENGTH 32u
#define FS_FANON_TILE 256u             /* positions a workgroup of the gram pass hashes      */
/* Counted per token of the corpus: 4 bytes (its gram's slot), 1 byte (its flags) and 2 bits
 * (the two cover masks); per slot of the gram table, S1 = the power of two at or above twice
 * the positions plus the scripts' grams, FS_FANON_SLOT_BYTES bytes (key, first, occurrences,
 * works, canon); per slot of the (gram, work) set, the power of two at or above twice the
 * positions, 8 bytes: between 63 and 121 bytes per token.  Once the passages are known: 20 bytes
 * per passage, and per slot of the phrase tables (the power of two at or above twice the
 * passages) FS_FANON_PHRASE_SLOT_BYTES bytes.  Their sum may be up to FS_FANON_MAX_BYTES, 8 GiB
 * where the siblings take 1 GiB because here the corpus itself is the input; the environment's
 * FS_FANON_MAX_BYTES replaces it. */
#define FS_FANON_SLOT_BYTES 21u
#define FS_FANON_PHRASE_SLOT_BYTES 32u
#define FS_FANON_MAX_BYTES (8ull << 30)

/* Host buffers in; n_works work records, up to cap_grams shared grams in order of first, up to
 * cap_passages passages in corpus order and up to cap_phrases phrases in order of first out, on
 * HIP device `device`.  n_positions and n_distinct (the positions with a gram and the distinct
 * grams of the fan works) may be null.  Both entry points: FS_E_INVALID for null arguments, k
 * outside FS_FANON_MIN_LENGTH..FS_FANON_MAX_LENGTH, min_works == 0, max_share outside 1..100,
 * a tok[i] >= n_ids, a canon id that is neither below n_ids nor FS_FANON_NO_ID, or offsets that
 * do not ascend from 0; FS_E_UNSUPPORTED for 2^32 tokens or more (script words included) or
 * tables above FS_FANON_MAX_BYTES (the message names the bytes needed and says to lower -n);
 * FS_E_CAPACITY with the three counts filled in when a cap is too small (the three buffers
 * untouched then, works complete).  A corpus without a position: n_tokens in the work records,
 * everything else 0, no kernel runs.
 * The environment's FS_FANON_HASH_BITS=k (a diagnostic, read once per call) keeps k bits of both
 * hashes (0: every key probes from slot 0); the output is the same. */
int fs_fanon(int device, const uint32_t* tok, const uint64_t* work_off, uint32_t n_works,
             uint32_t n_ids, const uint32_t* canon, const uint64_t* canon_off,
             uint32_t n_scripts, uint32_t k, uint32_t min_works, uint32_t max_share,
             fs_fanon_work* works, fs_fanon_gram* grams, uint64_t cap_grams,
             fs_fanon_passage* passages, uint64_t cap_passages, fs_fanon_phrase* phrases,
             uint64_t cap_phrases, uint64_t* n_grams, uint64_t* n_passages, uint64_t* n_phrases,
             uint64_t* n_positions, uint64_t* n_distinct);
/* The same over device-resident ids and offsets (n_tok = d_work_off[n_works] and n_canon =
 * d_canon_off[n_scripts] say how many ids the two buffers hold) into device buffers; returns
 * when they are written. */
int fs_fanon_dev(int device, const uint32_t* d_tok, uint64_t n_tok, const uint64_t* d_work_off,
                 uint32_t n_works, uint32_t n_ids, const uint32_t* d_canon, uint64_t n_canon,
                 const uint64_t* d_canon_off, uint32_t n_scripts, uint32_t k, uint32_t min_works,
                 uint32_t max_share, fs_fanon_work* d_works, fs_fanon_gram* d_grams,
                 uint64_t cap_grams, fs_fanon_passage* d_passages, uint64_t cap_passages,
                 fs_fanon_phrase* d_phrases, uint64_t cap_phrases, uint64_t* n_grams,
                 uint64_t* n_passages, uint64_t* n_phrases, uint64_t* n_positions,
                 uint64_t* n_distinct);
/* HIP-event milliseconds of the last fs_fanon / fs_fanon_dev call on this thread: insert (the
 * scripts' grams, then every position hashed and entered), flag (flags, cover masks, run heads
 * and their scans), phrases (least, most, the phrase table), place (the phrase order and the
 * gram, passage and phrase records), works (the work records), copy out, and the total of the
 * six; 0 for a pass that did not run.  tools/fanon_bench.py. */
int fs_fanon_times(double* ms);

/* Diagnostics (FS_DIAG=2 in the environment at fs_index_create): per wave range of the
 * last k_scan_rows launch on stream `lane`, eight uint64 {entry, filter staged, scan done,
 * rounds done, finished (ticks of the 100 MHz constant clock), rounds, flushes, records}.
 * *n = words available; FS_E_CAPACITY when cap is smaller.  tools/scan_timeline.py. */
int fs_debug_stamps(fs_index* ix, uint32_t lane, uint64_t* out, uint64_t cap, uint64_t* n);

/* Diagnostics, no GPU involved: out[0 .. n) = the ids of the window at position p of a 16-bit
 * id array, n = 2..8, taken the way the search's verification takes them from a batch's 16-bit
 * copy: the 32-bit words from the even position p & ~1 on, shifted down by one id when p is
 * odd.  Reads 8 ids from there (n = 8: 10), which the caller's array must hold (the device copy
 * is padded with zeroed ids).  tests/test_ids16_window.py. */
int fs_debug_ids16_window(const uint16_t* ids, uint64_t p, uint32_t n, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* FANDOM_SEARCH_H */
