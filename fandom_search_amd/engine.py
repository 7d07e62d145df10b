"""Python face of the C ABI: script index, device-resident corpus, search.

`ScriptIndex` stands where AnnIndexSearch.__init__ / build_lsh_engine stand in
the reference (/root/reference/search.py:131-154, 86-124); `Corpus` is a batch
of tokenised works already in HBM; `ScriptIndex.search` is
AnnIndexSearch.search (search.py:163-226) over the whole batch and returns the
numeric half of the records (abi.ROW_DTYPE), sorted by (work, fan word index).
"""

import ctypes as C
import weakref

import numpy as np

import atexit

from . import _lib, abi
from .vocab import pack_strings

# Handles still open when the interpreter exits are closed before the HIP runtime's
# own teardown (a __del__ that runs after it would call into a runtime that is gone).
_LIVE = weakref.WeakSet()


@atexit.register
def _close_all():
    for obj in sorted(_LIVE, key=lambda o: 0 if isinstance(o, ScriptIndex) else 1):
        try:
            obj.close()            # an index closes its corpora first
        except Exception:
            pass



class Corpus(object):
    def __init__(self, index, tok_vec, work_off, str_chars, str_off,
                 tok_str=None):
        self.index = index
        self.tok_vec = abi.as_u32(tok_vec)
        self.tok_str = abi.as_u32(tok_str) if tok_str is not None else None
        self.work_off = abi.as_u64(work_off)
        chars = abi.as_u32(str_chars)
        off = abi.as_u64(str_off)
        self.n_works = len(self.work_off) - 1
        self.n_tok = int(self.work_off[-1])
        if self.tok_vec.size < self.n_tok:
            raise ValueError("token buffer shorter than work_off[-1]")
        self._h = C.c_void_p()
        L = _lib.load()
        _lib.check(L.fs_corpus_create(
            index._h, abi.ptr(self.tok_vec, C.c_uint32),
            abi.ptr(self.tok_str, C.c_uint32),
            abi.ptr(self.work_off, C.c_uint64), self.n_works,
            abi.ptr(chars, C.c_uint32), abi.ptr(off, C.c_uint64),
            len(off) - 1, C.byref(self._h)), "fs_corpus_create")
        index._corpora.add(self)
        self._views = weakref.WeakSet()        # live CorpusView objects of this corpus
        _LIVE.add(self)

    def update_begin(self, tok_vec, work_off, tok_str=None):
        """Queue the upload of a new batch of works into this corpus (copy
        stream; returns at once).  The arrays must stay alive and untouched until
        update_end() or the next search on this corpus; pass pinned arrays
        (`pinned_array`) for the copy to overlap a running search."""
        self.tok_vec = abi.as_u32(tok_vec)
        self.tok_str = abi.as_u32(tok_str) if tok_str is not None else None
        self.work_off = abi.as_u64(work_off)
        self.n_works = len(self.work_off) - 1
        self.n_tok = int(self.work_off[-1])
        _lib.check(_lib.load().fs_corpus_update_begin(
            self._h, abi.ptr(self.tok_vec, C.c_uint32), abi.ptr(self.tok_str, C.c_uint32),
            abi.ptr(self.work_off, C.c_uint64), self.n_works), "fs_corpus_update_begin")

    def update_end(self):
        _lib.check(_lib.load().fs_corpus_update_end(self._h), "fs_corpus_update_end")

    def close(self):
        """Closes the views of this corpus first (the library would only detach them)."""
        for v in list(getattr(self, "_views", ())):
            v.close()
        if self._h:
            _lib.load().fs_corpus_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CorpusView(object):
    """The works of another index's Corpus, searched by `index` without a second upload
    (fs_corpus_view): ScriptIndex.search / search_begin / search_end take it like a Corpus.
    Sizes are the base's as they stand; a new batch goes in through the base's update_begin."""

    def __init__(self, index, base):
        if not isinstance(base, Corpus):
            raise TypeError("the base of a view is a Corpus")
        self.index = index
        self.base = base
        self._h = C.c_void_p()
        _lib.check(_lib.load().fs_corpus_view(index._h, base._h, C.byref(self._h)), "fs_corpus_view")
        index._corpora.add(self)
        base._views.add(self)
        _LIVE.add(self)

    n_tok = property(lambda self: self.base.n_tok)
    n_works = property(lambda self: self.base.n_works)
    work_off = property(lambda self: self.base.work_off)

    def update_begin(self, tok_vec, work_off, tok_str=None):
        raise ValueError("a corpus view is updated through its base corpus")

    def update_end(self):
        raise ValueError("a corpus view is updated through its base corpus")

    def close(self):
        # (also after the base has gone: the library only frees the view's own tables)
        if self._h:
            _lib.load().fs_corpus_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def torch_ready():
    """The library launches on streams of its own (hipStreamNonBlocking: no implicit ordering
    with torch's stream).  Device memory that torch has only just produced -- a zero-filled
    buffer, a host-to-device copy, a clone -- must be complete before it is handed to a call
    that reads it or writes into it: otherwise the library's kernel can read what the allocator
    left there from an earlier batch, or torch's fill can land on top of the library's records.
    (Round 5: `unpack_shard` read a stale copy of a shard's work offsets once in five runs of the
    two-rank test and attributed a run of records to the work in front.)  Not for per-step paths:
    buffers made ahead of time need none of this."""
    import sys
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.current_stream().synchronize()


def _first_cap(cap, out_ptrs, first):
    """The capacity a *_device method begins with: the caller's `cap`; without one, `first`
    for buffers of the method's own and 0 for the caller's."""
    if cap is None:
        return 0 if out_ptrs is not None else first
    return int(cap)


def _rows_call(where, call, fixed, grown, caps, out_ptrs, message):
    """The fs_*_rows call behind a *_device method of ScriptIndex.  call(fixed, grown, caps,
    counts) makes it: the device addresses of the fixed outputs, those of the growing outputs,
    their capacities, and one c_uint64 per growing output for the count the library reports.
    `fixed` lists (count, dtype) per fixed output, `grown` the growing outputs' dtypes, `caps`
    their capacities.  With `out_ptrs` (the caller's buffers, the fixed ones first): one call
    and the count (the counts, as a tuple, of several growing outputs); FsError(FS_E_CAPACITY)
    saying `message`, with the same in .required, when a buffer is too small.  Without:
    buffers from torch, the growing ones enlarged to the reported counts until the call fits,
    and the outputs as a tuple of host arrays, the fixed ones first."""
    counts = [C.c_uint64(0) for _ in grown]
    if out_ptrs is not None:
        rc = call(out_ptrs[:len(fixed)], out_ptrs[len(fixed):], caps, counts)
        got = int(counts[0].value) if len(counts) == 1 else tuple(int(c.value) for c in counts)
        if rc == abi.FS_E_CAPACITY:
            err = _lib.FsError(rc, where, message)
            err.required = got
            raise err
        _lib.check(rc, where)
        return got
    import torch

    def device(count, dtype):
        return torch.empty(max(1, int(count)) * np.dtype(dtype).itemsize, dtype=torch.uint8,
                           device="cuda")

    def host(buf, count, dtype):
        return buf[:int(count) * np.dtype(dtype).itemsize].cpu().numpy().view(dtype)
    held = [device(n, d) for n, d in fixed]
    caps = [int(c) for c in caps]
    while True:
        room = [device(c, d) for c, d in zip(caps, grown)]
        torch_ready()
        rc = call([b.data_ptr() for b in held], [b.data_ptr() for b in room], caps, counts)
        if rc == abi.FS_E_CAPACITY:                      # (the library says how many)
            caps = [max(c, int(n.value)) for c, n in zip(caps, counts)]
            continue
        _lib.check(rc, where)
        return tuple([host(b, n, d) for b, (n, d) in zip(held, fixed)]
                     + [host(b, n.value, d) for b, n, d in zip(room, counts, grown)])


class PinnedBuffer(object):
    """Page-locked host memory (hipHostMalloc) viewed as a numpy array."""

    def __init__(self, count, dtype):
        self.dtype = np.dtype(dtype)
        self._p = C.c_void_p()
        nbytes = max(1, int(count)) * self.dtype.itemsize
        _lib.check(_lib.load().fs_host_alloc(nbytes, C.byref(self._p)), "fs_host_alloc")
        buf = (C.c_char * nbytes).from_address(self._p.value)
        self.array = np.frombuffer(buf, dtype=self.dtype, count=int(count))

    def close(self):
        if self._p:
            self.array = None
            _lib.load().fs_host_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def search_stream(index, batches, str_chars, str_off):
    """Search a corpus that arrives batch by batch (BASELINE configs[4]).

    `batches` yields (tok_vec, work_off) pairs, or (tok_vec, work_off, tok_str).
    Two device corpora alternate: while batch i is searched, batch i+1 is copied
    to the GPU on the other corpus's copy stream.  Yields (rows, stats) per batch,
    work indices local to the batch; the rows are a view of a buffer that the next batch
    overwrites (ScriptIndex.search(reuse=True))."""
    it = iter(batches)
    slots = [None, None]
    cur = None

    def stage(slot, batch):
        tok_str = batch[2] if len(batch) > 2 else None
        if slots[slot] is None:
            slots[slot] = index.corpus(batch[0], batch[1], str_chars, str_off, tok_str=tok_str)
        else:
            slots[slot].update_begin(batch[0], batch[1], tok_str=tok_str)

    try:
        first = next(it)
    except StopIteration:
        return
    stage(0, first)
    cur = 0
    while cur is not None:
        nxt_batch = next(it, None)
        nxt = None
        if nxt_batch is not None:
            nxt = cur ^ 1
            stage(nxt, nxt_batch)            # queued; overlaps the search below
        yield index.search(slots[cur], reuse=True)
        cur = nxt
    for c in slots:
        if c is not None:
            c.close()


class ScriptIndex(object):
    def __init__(self, script_vec, script_words, emb, normals, cfg=None,
                 **cfg_kw):
        L = _lib.load()
        self.cfg = cfg or abi.make_config(**cfg_kw)
        sv = abi.as_u32(script_vec)
        chars, off = pack_strings(list(script_words))
        if len(off) - 1 != len(sv):
            raise ValueError("one word per script token expected")
        emb = np.ascontiguousarray(emb, dtype=np.float32)
        if emb.ndim != 2 or emb.shape[1] != self.cfg.emb_dim:
            raise ValueError("embedding must be (V, %d)" % self.cfg.emb_dim)
        normals = np.ascontiguousarray(normals, dtype=np.float64)
        want = (self.cfg.number_of_hashes * self.cfg.hash_dimensions
                * self.cfg.emb_dim * self.cfg.window_size)
        if normals.size != want:
            raise ValueError("normals must hold H*B*D*n = %d values" % want)
        self._corpora = weakref.WeakSet()      # live Corpus objects of this index
        _LIVE.add(self)
        self._h = C.c_void_p()
        _lib.check(L.fs_index_create(
            C.byref(self.cfg), abi.ptr(sv, C.c_uint32),
            abi.ptr(chars, C.c_uint32), abi.ptr(off, C.c_uint64), len(sv),
            abi.ptr(emb, C.c_float), emb.shape[0],
            abi.ptr(normals, C.c_double), C.byref(self._h)),
            "fs_index_create")
        info = abi.FsIndexInfo()
        _lib.check(L.fs_index_info_get(self._h, C.byref(info)),
                   "fs_index_info_get")
        self.info = info.as_dict()

    def corpus(self, tok_vec, work_off, str_chars, str_off, tok_str=None):
        return Corpus(self, tok_vec, work_off, str_chars, str_off, tok_str)

    def corpus_view(self, base):
        """A corpus of this index over the works of `base`, a Corpus of another index on the
        same device with the same window size, emb_dim and vector table (fs_corpus_view)."""
        return CorpusView(self, base)

    def search(self, corpus, cap=None, reuse=False):
        """Rows (numpy structured array, host) and stats of one batch.  `reuse`: the rows
        are a view of a buffer the index keeps and writes again on its next search with
        `reuse` (a fresh 40 MB array per call costs more in page faults than the copy over
        PCIe); take a copy of what must outlive that."""
        L = _lib.load()
        st = abi.FsStats()
        n = C.c_uint64(0)
        cap = int(cap) if cap else max(1024, corpus.n_tok // 16)
        while True:
            if reuse:
                if getattr(self, "_rows_buf", None) is None or len(self._rows_buf) < cap:
                    self._rows_buf = np.empty(cap, dtype=abi.ROW_DTYPE)
                rows = self._rows_buf
                cap = len(rows)
            else:
                rows = np.empty(cap, dtype=abi.ROW_DTYPE)
            rc = L.fs_search_corpus(self._h, corpus._h,
                                    rows.ctypes.data_as(C.c_void_p), cap, 0,
                                    C.byref(n), C.byref(st))
            if rc == abi.FS_E_CAPACITY:
                cap = int(n.value)
                continue
            _lib.check(rc, "fs_search_corpus")
            return rows[:n.value], st

    @staticmethod
    def _rows_mode(packed):
        """packed: False (32-byte fs_row), True or 16 (16-byte wire records), 8
        (8-byte wire records)."""
        if packed == 8:
            return abi.FS_ROWS_DEVICE_PACKED8
        return abi.FS_ROWS_DEVICE_PACKED if packed else abi.FS_ROWS_DEVICE

    def search_device(self, corpus, rows_ptr, cap, packed=False):
        """Rows written to a caller-owned device buffer (`rows_ptr`: 16-byte
        aligned address on this index's device, `cap` records of 32 bytes, or of
        16 / 8 bytes when `packed` is True / 8: the wire formats of the exact
        pipeline, see unpack_device / unpack8_device).  Returns (n_rows, stats);
        raises FsError(FS_E_CAPACITY) with .required when the buffer is too small."""
        L = _lib.load()
        st = abi.FsStats()
        n = C.c_uint64(0)
        mode = self._rows_mode(packed)
        rc = L.fs_search_corpus(self._h, corpus._h, C.c_void_p(rows_ptr),
                                int(cap), mode, C.byref(n), C.byref(st))
        if rc == abi.FS_E_CAPACITY:
            err = _lib.FsError(rc, "fs_search_corpus", "row buffer too small")
            err.required = int(n.value)
            raise err
        _lib.check(rc, "fs_search_corpus")
        return int(n.value), st

    def set_scan_timing(self, period):
        """Attach timing events to every `period`-th scan launch only."""
        _lib.check(_lib.load().fs_index_set_scan_timing(self._h, int(period)),
                   "fs_index_set_scan_timing")

    def kernel_name(self, corpus):
        """Diagnostics: the kernel that dominates a search of `corpus` (profile name)."""
        return _lib.load().fs_search_kernel_name(self._h, corpus._h).decode()

    def scan_shape(self, corpus):
        """Diagnostics: what a search of `corpus` would launch (fs_index_scan_shape), as a dict:
        waves and blocks of k_scan_rows (0: the chained kernels), filter_log2_words,
        seeds_lds_bytes, log2_buckets, log2_slots, overflow_buckets, wide_buckets, host_wire8."""
        out = abi.FsScanShape()
        _lib.check(_lib.load().fs_index_scan_shape(self._h, corpus._h, C.byref(out)), "fs_index_scan_shape")
        return out.as_dict()

    def scan_ids16(self, corpus):
        """Diagnostics: whether a search of `corpus` streams the 16-bit copy of its ids through
        k_scan_rows (fs_scan_shape.ids16: every vector id below 2^16, no string ids of the batch's
        own, FS_SCAN_IDS16 not 0) instead of the 32-bit ids."""
        out = abi.FsScanShape()
        _lib.check(_lib.load().fs_index_scan_shape(self._h, corpus._h, C.byref(out)), "fs_index_scan_shape")
        return bool(out.ids16)

    def stream_floor(self, corpus, reps=20):
        """Diagnostics: ms of a kernel that only reads `corpus`' ids in k_scan_rows' launch
        shape (fs_stream_floor)."""
        ms = C.c_double()
        _lib.check(_lib.load().fs_stream_floor(self._h, corpus._h, reps, C.byref(ms)), "fs_stream_floor")
        return ms.value

    def component_sizes(self):
        """Diagnostics: (sizes of the components of near vectors, whether the prefilters use
        them) -- fs_index_component_sizes."""
        n, used = C.c_uint64(), C.c_uint32()
        L = _lib.load()
        _lib.check(L.fs_index_component_sizes(self._h, None, 0, C.byref(n), C.byref(used)), "fs_index_component_sizes")
        sizes = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            _lib.check(L.fs_index_component_sizes(self._h, abi.ptr(sizes, C.c_uint32), n.value, C.byref(n),
                                                  C.byref(used)), "fs_index_component_sizes")
        return sizes, bool(used.value)

    def share_info(self):
        """Diagnostics: the share rule of the LSH pipeline on this index (fs_index_share_info):
        {"flags", "components", "largest", "gamma"}; flags 0 = not in use."""
        f, n, m, g = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_double()
        _lib.check(_lib.load().fs_index_share_info(self._h, C.byref(f), C.byref(n), C.byref(m), C.byref(g)),
                   "fs_index_share_info")
        return {"flags": f.value, "components": n.value, "largest": m.value, "gamma": g.value}

    def share_counts(self):
        """Diagnostics (FS_SHARE_COUNT=1 when the index was built): what passed what in k_share_scan
        since the last call -- fs_index_share_counts."""
        out = (C.c_uint64 * 8)()
        _lib.check(_lib.load().fs_index_share_counts(self._h, out), "fs_index_share_counts")
        names = ("windows", "windows_with_a_key_in_the_filter", "map_entries", "pairs_tested", "distances",
                 "windows_flagged", "windows_flagged_as_they_are")
        return {k: int(out[i]) for i, k in enumerate(names)}

    LSH_COUNT_NAMES = (
        "record_with_neighbours", "record_alone", "wmap_ended_0", "wmap_ended_1", "wmap_ended_2",
        "wmap_pending_distance", "wmap_pending_many", "wmap_pending_full_bucket",
        "enum_listed_1", "enum_listed_2", "enum_listed_3", "enum_listed_4", "enum_reordered", "enum_cut",
        "enum_chain_once", "enum_chain_twice", "enum_giveup_fifth", "enum_giveup_chain", "enum_giveup_tie")

    def lsh_counts(self):
        """Diagnostics (FS_LSH_COUNT=1 when the index was built): windows by the branch they took in
        the kernels that read the one-slot maps (second stage of k_lsh_sift / k_lsh_sift2, k_lsh_enum)
        since the last call -- fs_index_lsh_counts."""
        out = (C.c_uint64 * abi.FS_LSH_COUNTERS)()
        _lib.check(_lib.load().fs_index_lsh_counts(self._h, out), "fs_index_lsh_counts")
        return {k: int(out[i]) for i, k in enumerate(self.LSH_COUNT_NAMES)}

    def profile(self, corpus, rows_ptr, cap):
        """Diagnostics: one search of `corpus` (records to the device buffer at `rows_ptr`)
        with a HIP event behind each of its kernels; returns [(kernel name, ms), ...] in
        launch order.  The GPU should be idle otherwise (fs_search_profile)."""
        names = C.create_string_buffer(2048)
        ms = (C.c_double * 32)()
        n = C.c_uint32()
        _lib.check(_lib.load().fs_search_profile(self._h, corpus._h, C.c_void_p(rows_ptr), cap, 1,
                                                 names, len(names), ms, 32, C.byref(n)),
                   "fs_search_profile")
        labels = names.value.decode().split("\n")
        return [(labels[i], float(ms[i])) for i in range(min(n.value, 32, len(labels) - 1))]

    def reload_switches(self):
        """Diagnostics: re-read the FS_* environment switches (read at creation)."""
        _lib.check(_lib.load().fs_index_reload_switches(self._h), "fs_index_reload_switches")

    def search_begin(self, corpus, rows_ptr, cap, packed=False, header=False):
        """Queue a search (rows to the device buffer at `rows_ptr`) and return a
        ticket for search_end; up to four may be in flight per index.  `header`:
        the buffer starts with a 32-byte header whose first eight bytes receive the
        record count, the `cap` records follow it."""
        t = C.c_uint32(0)
        mode = self._rows_mode(packed) | (abi.FS_ROWS_HEADER if header else 0)
        _lib.check(_lib.load().fs_search_corpus_begin(
            self._h, corpus._h, C.c_void_p(rows_ptr), int(cap), mode, C.byref(t)),
            "fs_search_corpus_begin")
        return t.value

    def search_end(self, ticket):
        """(n_rows, stats) of a queued search; FsError(FS_E_CAPACITY).required when
        the row buffer was too small."""
        st = abi.FsStats()
        n = C.c_uint64(0)
        rc = _lib.load().fs_search_corpus_end(self._h, int(ticket), C.byref(n), C.byref(st))
        if rc == abi.FS_E_CAPACITY:
            err = _lib.FsError(rc, "fs_search_corpus_end", "row buffer too small")
            err.required = int(n.value)
            raise err
        _lib.check(rc, "fs_search_corpus_end")
        return int(n.value), st

    def unpack_device(self, packed_ptr, n, rows_ptr):
        """Expand `n` 16-byte wire records at device address `packed_ptr` into
        fs_row records at `rows_ptr` (both on this index's device)."""
        _lib.check(_lib.load().fs_rows_unpack(self._h, C.c_void_p(packed_ptr), int(n),
                                              C.c_void_p(rows_ptr)), "fs_rows_unpack")

    def unpack8_device(self, packed_ptr, n, work_off_ptr, n_works, rows_ptr):
        """Expand `n` 8-byte wire records; `work_off_ptr`: device address of the
        n_works + 1 uint64 work offsets of the batch the records come from."""
        _lib.check(_lib.load().fs_rows_unpack8(self._h, C.c_void_p(packed_ptr), int(n),
                                               C.c_void_p(work_off_ptr), int(n_works),
                                               C.c_void_p(rows_ptr)), "fs_rows_unpack8")

    def reuse_histogram_device(self, rows_ptr, n_rows, thresholds):
        """`format` aggregation over device-resident fs_row records (after a
        search or a gather): counts[n_script][len(thresholds) + 1] on the host."""
        import torch
        thr = np.ascontiguousarray(thresholds, dtype=np.float64)
        n_script = int(self.info["n_script"])
        out = torch.zeros(max(1, n_script) * (len(thr) + 1), dtype=torch.int32, device="cuda")
        torch_ready()                       # (the zeros are there before the kernel adds to them)
        _lib.check(_lib.load().fs_reuse_histogram_rows(
            self._h, C.c_void_p(rows_ptr), int(n_rows), abi.ptr(thr, C.c_double), len(thr),
            C.c_void_p(out.data_ptr())), "fs_reuse_histogram_rows")
        return out.cpu().numpy().view(np.uint32)[:n_script * (len(thr) + 1)] \
            .reshape(n_script, len(thr) + 1)

    def passages_device(self, rows_ptr, n_rows, min_words=6, max_gap=0, out_ptr=None, cap=0):
        """`passages` over device-resident fs_row records sorted by (work, fan_ix) (after a
        search or a gather; fs_passages_rows).  Without `out_ptr`: the passages as a host
        abi.PASSAGE_DTYPE array.  With `out_ptr` (a device buffer of `cap` passages): their
        number; FsError(FS_E_CAPACITY) with .required when the buffer is too small.  A buffer
        torch has only just produced goes in after torch_ready()."""
        L = _lib.load()

        def call(_, grown, caps, counts):
            return L.fs_passages_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(min_words),
                                      int(max_gap), C.c_void_p(grown[0]), int(caps[0]),
                                      C.byref(counts[0]))
        if out_ptr is not None:
            return _rows_call("fs_passages_rows", call, [], [abi.PASSAGE_DTYPE], [cap], [out_ptr],
                              "passage buffer too small")
        cap = int(n_rows) // max(1, int(min_words)) + 1      # passages never outnumber this
        return _rows_call("fs_passages_rows", call, [], [abi.PASSAGE_DTYPE], [cap], None,
                          "passage buffer too small")[0]

    def works_device(self, rows_ptr, n_rows, n_works, group_of=None, n_groups=0, min_words=6,
                     max_gap=0, thresholds=None, out_ptrs=None, cap=0):
        """`works` over device-resident fs_row records sorted by (work, fan_ix) (after a search
        or a gather; fs_works_rows): per-work summaries, threshold counts and the (work, group)
        cells for the host map `group_of` (script word -> group id < n_groups; None: no
        groups).  Without `out_ptrs`: (abi.WORK_DTYPE[n_works], counts[n_works][n_thr + 1],
        abi.WORK_CELL_DTYPE[n_cells]) on the host.  With `out_ptrs` = device addresses
        (summaries, counts, cells; the last a buffer of `cap` cells): the number of cells;
        FsError(FS_E_CAPACITY) with .required when that buffer is too small.  Buffers torch
        has only just produced go in after torch_ready()."""
        from .format import THRESHOLDS
        L = _lib.load()
        thr = np.ascontiguousarray(THRESHOLDS if thresholds is None else thresholds,
                                   dtype=np.float64)
        gmap = None if group_of is None else abi.as_u32(group_of)
        n_works, cols = int(n_works), len(thr) + 1

        def call(fixed, grown, caps, counts):
            return L.fs_works_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), n_works,
                                   abi.ptr(gmap, C.c_uint32), int(n_groups), int(min_words),
                                   int(max_gap), abi.ptr(thr, C.c_double), len(thr),
                                   C.c_void_p(fixed[0]), C.c_void_p(fixed[1]),
                                   C.c_void_p(grown[0]), int(caps[0]), C.byref(counts[0]))
        if out_ptrs is None:
            cap = min(int(n_rows), n_works * int(n_groups))  # a record makes at most one cell
        got = _rows_call("fs_works_rows", call,
                         [(n_works, abi.WORK_DTYPE), (n_works * cols, np.uint32)],
                         [abi.WORK_CELL_DTYPE], [cap], out_ptrs, "cell buffer too small")
        if out_ptrs is not None:
            return got
        return got[0], got[1].reshape(n_works, cols), got[2]

    def quotes_device(self, rows_ptr, n_rows, n_works, min_words=6, max_gap=0, min_works=1,
                      out_ptrs=None, cap=0):
        """`quotes` over device-resident fs_row records sorted by (work, fan_ix) (after a search
        or a gather; fs_quotes_rows): the script's words with the works and passages behind
        them, and the regions of depth >= min_works.  Without `out_ptrs`:
        (abi.QUOTE_WORD_DTYPE[n_script], abi.QUOTE_REGION_DTYPE[n_regions]) on the host.  With
        `out_ptrs` = device addresses (words; regions, a buffer of `cap` of them): the number of
        regions; FsError(FS_E_CAPACITY) with .required when that buffer is too small (the words
        are complete then).  Buffers torch has only just produced go in after torch_ready()."""
        L = _lib.load()
        n_script = int(self.info["n_script"])

        def call(fixed, grown, caps, counts):
            return L.fs_quotes_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                    int(min_words), int(max_gap), int(min_works),
                                    C.c_void_p(fixed[0]), C.c_void_p(grown[0]), int(caps[0]),
                                    C.byref(counts[0]))
        if out_ptrs is None:
            cap = min(int(n_rows), (n_script + 1) // 2)      # regions lie a word apart at least
        return _rows_call("fs_quotes_rows", call, [(n_script, abi.QUOTE_WORD_DTYPE)],
                          [abi.QUOTE_REGION_DTYPE], [cap], out_ptrs, "region buffer too small")

    def pairs_device(self, rows_ptr, n_rows, n_works, min_words=6, max_gap=0, min_shared=6,
                     out_ptrs=None, cap=None):
        """`pairs` over device-resident fs_row records sorted by (work, fan_ix) (after a search
        or a gather; fs_pairs_rows): per work its coverage, partners and best partner, and the
        pairs of works sharing >= min_shared script words, in (a, b) order.  Without
        `out_ptrs`: (abi.PAIR_WORK_DTYPE[n_works], abi.PAIR_DTYPE[n_pairs]) on the host.  With
        `out_ptrs` = device addresses (works; pairs, a buffer of `cap` of them): the number of
        pairs; FsError(FS_E_CAPACITY) with .required when that buffer is too small (the works
        are complete then).  Buffers torch has only just produced go in after torch_ready()."""
        L = _lib.load()

        def call(fixed, grown, caps, counts):
            return L.fs_pairs_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                   int(min_words), int(max_gap), int(min_shared),
                                   C.c_void_p(fixed[0]), C.c_void_p(grown[0]), int(caps[0]),
                                   C.byref(counts[0]))
        return _rows_call("fs_pairs_rows", call, [(n_works, abi.PAIR_WORK_DTYPE)],
                          [abi.PAIR_DTYPE], [_first_cap(cap, out_ptrs, 4096)], out_ptrs,
                          "pair buffer too small")

    def companions_device(self, rows_ptr, n_rows, n_works, unit_of_ptr, n_units, min_words=6,
                          max_gap=0, min_both=2, min_share=0, out_ptrs=None, cap=None):
        """`companions` over device-resident fs_row records sorted by (work, fan_ix) and a
        device-resident unit map of the script's words (fs_companions_rows): per unit its works,
        partners and best partner, and the pairs of units that >= min_both works quote both,
        in (a, b) order.  Without `out_ptrs`: (abi.COMPANION_UNIT_DTYPE[n_units],
        abi.COMPANION_DTYPE[n_pairs]) on the host.  With `out_ptrs` = device addresses (units;
        pairs, a buffer of `cap` of them): the number of pairs; FsError(FS_E_CAPACITY) with
        .required when that buffer is too small (the units are complete then).  Buffers torch
        has only just produced go in after torch_ready()."""
        L = _lib.load()

        def call(fixed, grown, caps, counts):
            return L.fs_companions_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                        C.c_void_p(unit_of_ptr), int(n_units), int(min_words),
                                        int(max_gap), int(min_both), int(min_share),
                                        C.c_void_p(fixed[0]), C.c_void_p(grown[0]), int(caps[0]),
                                        C.byref(counts[0]))
        return _rows_call("fs_companions_rows", call, [(n_units, abi.COMPANION_UNIT_DTYPE)],
                          [abi.COMPANION_DTYPE], [_first_cap(cap, out_ptrs, 4096)], out_ptrs,
                          "pair buffer too small")

    def bundles_device(self, rows_ptr, n_rows, n_works, unit_of_ptr, n_units, min_words=6,
                       max_gap=0, min_all=5, max_size=4, out_ptrs=None, cap=None):
        """`bundles` over device-resident fs_row records sorted by (work, fan_ix) and a
        device-resident unit map of the script's words (fs_bundles_rows): per unit its works and
        the listed sets holding it, per size 2 .. max_size + 1 the level's counts, and every set
        of 2 .. max_size units that >= min_all works quote in full, by size, then
        lexicographically.  Without `out_ptrs`: (abi.BUNDLE_UNIT_DTYPE[n_units],
        abi.BUNDLE_LEVEL_DTYPE[max_size], abi.BUNDLE_DTYPE[n_sets]) on the host.  With `out_ptrs`
        = device addresses (units; levels; sets, a buffer of `cap` of them): the number of
        sets; FsError(FS_E_CAPACITY) with .required when that buffer is too small (the units
        and the levels are complete then).  Buffers torch has only just produced go in after
        torch_ready()."""
        L = _lib.load()

        def call(fixed, grown, caps, counts):
            return L.fs_bundles_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                     C.c_void_p(unit_of_ptr), int(n_units), int(min_words),
                                     int(max_gap), int(min_all), int(max_size),
                                     C.c_void_p(fixed[0]), C.c_void_p(fixed[1]),
                                     C.c_void_p(grown[0]), int(caps[0]), C.byref(counts[0]))
        return _rows_call("fs_bundles_rows", call,
                          [(n_units, abi.BUNDLE_UNIT_DTYPE),
                           (max(1, int(max_size)), abi.BUNDLE_LEVEL_DTYPE)],
                          [abi.BUNDLE_DTYPE], [_first_cap(cap, out_ptrs, 4096)], out_ptrs,
                          "set buffer too small")

    def routes_device(self, rows_ptr, n_rows, n_works, unit_of_ptr, n_units, min_words=6,
                      max_gap=0, max_skip=abi.FS_NONE, min_all=5, max_length=4, out_ptrs=None,
                      cap=None):
        """`routes` over device-resident fs_row records sorted by (work, fan_ix) and a
        device-resident unit map of the script's words (fs_routes_rows): per unit its works and
        the listed routes holding it, per length 2 .. max_length + 1 the level's counts, and
        every route of 2 .. max_length units that >= min_all works quote in that order, at most
        max_skip elements between two of its units (abi.FS_NONE: any distance), by length, then
        lexicographically.  Without `out_ptrs`: (abi.ROUTE_UNIT_DTYPE[n_units],
        abi.ROUTE_LEVEL_DTYPE[max_length], abi.ROUTE_DTYPE[n_routes]) on the host.  With
        `out_ptrs` = device addresses (units; levels; routes, a buffer of `cap` of them): the
        number of routes; FsError(FS_E_CAPACITY) with .required when that buffer is too small
        (the units and the levels are complete then).  Buffers torch has only just produced go
        in after torch_ready()."""
        L = _lib.load()

        def call(fixed, grown, caps, counts):
            return L.fs_routes_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                    C.c_void_p(unit_of_ptr), int(n_units), int(min_words),
                                    int(max_gap), int(max_skip), int(min_all), int(max_length),
                                    C.c_void_p(fixed[0]), C.c_void_p(fixed[1]),
                                    C.c_void_p(grown[0]), int(caps[0]), C.byref(counts[0]))
        return _rows_call("fs_routes_rows", call,
                          [(n_units, abi.ROUTE_UNIT_DTYPE),
                           (max(1, int(max_length)), abi.ROUTE_LEVEL_DTYPE)],
                          [abi.ROUTE_DTYPE], [_first_cap(cap, out_ptrs, 4096)], out_ptrs,
                          "route buffer too small")

    def lines_device(self, rows_ptr, n_rows, n_works, line_first_ptr, n_lines, min_words=6,
                     max_gap=0, most=50, out_ptrs=None, caps=None):
        """`lines` over device-resident fs_row records sorted by (work, fan_ix) and a
        device-resident line table of n_lines + 1 entries (fs_lines_rows): per line the works
        quoting it and how completely, per active work its lines, and the cells (line, work) in
        that order.  Without `out_ptrs`: (abi.LINE_DTYPE[n_lines], abi.LINE_WORK_DTYPE[active
        works], abi.LINE_CELL_DTYPE[n_cells]) on the host.  With `out_ptrs` = device addresses
        (lines; works, cells, buffers of `caps` = (works, cells) of them): (active works,
        cells); FsError(FS_E_CAPACITY) with .required = both counts when a buffer is too small
        (the lines are complete then).  Buffers torch has only just produced go in after
        torch_ready()."""
        L = _lib.load()

        def call(fixed, grown, caps, counts):
            return L.fs_lines_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                   C.c_void_p(line_first_ptr), int(n_lines), int(min_words),
                                   int(max_gap), int(most), C.c_void_p(fixed[0]),
                                   C.c_void_p(grown[0]), int(caps[0]), C.byref(counts[0]),
                                   C.c_void_p(grown[1]), int(caps[1]), C.byref(counts[1]))
        if caps is None:
            caps = (0, 0) if out_ptrs is not None else (256, 4096)
        return _rows_call("fs_lines_rows", call, [(n_lines, abi.LINE_DTYPE)],
                          [abi.LINE_WORK_DTYPE, abi.LINE_CELL_DTYPE], list(caps), out_ptrs,
                          "work or cell buffer too small")

    def fragments_device(self, rows_ptr, n_rows, n_works, min_words=6, max_gap=0, min_works=2,
                         min_length=3, max_words=128, out_ptrs=None, caps=None):
        """`fragments` over device-resident fs_row records sorted by (work, fan_ix)
        (fs_fragments_rows): the closed frequent intervals of the script in (words, first)
        order, and per active work its runs and the fragments they hold.  Without `out_ptrs`:
        (abi.FRAGMENT_DTYPE[n_frags], abi.FRAGMENT_WORK_DTYPE[active works]) on the host.  With
        `out_ptrs` = device addresses (fragments, works, buffers of `caps` = (fragments, works)
        of them): (fragments, active works); FsError(FS_E_CAPACITY) with .required = both
        counts when a buffer is too small (both untouched then).  Buffers torch has only just
        produced go in after torch_ready()."""
        L = _lib.load()

        def call(fixed, grown, caps, counts):
            return L.fs_fragments_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                       int(min_words), int(max_gap), int(min_works),
                                       int(min_length), int(max_words), C.c_void_p(grown[0]),
                                       int(caps[0]), C.byref(counts[0]), C.c_void_p(grown[1]),
                                       int(caps[1]), C.byref(counts[1]))
        if caps is None:
            caps = (0, 0) if out_ptrs is not None else (4096, 256)
        return _rows_call("fs_fragments_rows", call, [], [abi.FRAGMENT_DTYPE,
                                                          abi.FRAGMENT_WORK_DTYPE], list(caps),
                          out_ptrs, "fragment or work buffer too small")

    def digest_device(self, rows_ptr, n_rows, n_works, min_words=6, max_gap=0, picks=0,
                      cover=100, min_gain=1, out_ptrs=None, caps=None):
        """`digest` over device-resident fs_row records sorted by (work, fan_ix)
        (fs_digest_rows): the greedy picks in pick order, per active work what the picks show
        of it, and TOTAL, the script words any work covers.  Without `out_ptrs`:
        (abi.DIGEST_PICK_DTYPE[picks made], abi.DIGEST_WORK_DTYPE[active works], TOTAL) on the
        host.  With `out_ptrs` = device addresses (picks, works, buffers of `caps` = (picks,
        works) of them): (picks made, active works, TOTAL); FsError(FS_E_CAPACITY) with
        .required = both counts when a buffer is too small (both untouched then).  Buffers torch
        has only just produced go in after torch_ready()."""
        L = _lib.load()
        total = C.c_uint64(0)

        def call(fixed, grown, caps, counts):
            return L.fs_digest_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                    int(min_words), int(max_gap), int(picks), int(cover),
                                    int(min_gain), C.c_void_p(grown[0]), int(caps[0]),
                                    C.byref(counts[0]), C.c_void_p(grown[1]), int(caps[1]),
                                    C.byref(counts[1]), C.byref(total))
        if caps is None:                    # (neither count is above the works)
            room = max(1, min(int(n_works), int(n_rows)))
            caps = (0, 0) if out_ptrs is not None else (room, room)
        got = _rows_call("fs_digest_rows", call, [], [abi.DIGEST_PICK_DTYPE,
                                                      abi.DIGEST_WORK_DTYPE], list(caps),
                         out_ptrs, "pick or work buffer too small")
        return tuple(got) + (int(total.value),)

    def intervals_device(self, rows_ptr, n_rows, n_works, unit_of_ptr, n_units, min_words=6,
                         max_gap=0, replicates=1000, seed=0, level=95, out_ptrs=None):
        """`intervals` over device-resident fs_row records sorted by (work, fan_ix) and a
        device-resident unit map of the script's words (fs_intervals_rows): per unit its works
        with the bootstrap's order statistics and its standing against the next unit, per
        replicate its totals.  Without `out_ptrs`: (abi.INTERVAL_UNIT_DTYPE[n_units],
        abi.INTERVAL_REPLICATE_DTYPE[replicates]) on the host.  With `out_ptrs` = device
        addresses (units, replicates): they are written and () comes back.  Buffers torch has
        only just produced go in after torch_ready()."""
        L = _lib.load()

        def call(fixed, grown, caps, counts):
            return L.fs_intervals_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                       C.c_void_p(unit_of_ptr), int(n_units), int(min_words),
                                       int(max_gap), int(replicates), int(seed), int(level),
                                       C.c_void_p(fixed[0]), C.c_void_p(fixed[1]))
        return _rows_call("fs_intervals_rows", call,
                          [(n_units, abi.INTERVAL_UNIT_DTYPE),
                           (replicates, abi.INTERVAL_REPLICATE_DTYPE)], [], [], out_ptrs, "")

    def contrast_device(self, rows_ptr, n_rows, n_works, unit_of_ptr, n_units, side_ptr,
                        min_words=6, max_gap=0, min_quoting=5, permutations=1000, seed=0,
                        key_bits=32, out_ptrs=None):
        """`contrast` over device-resident fs_row records sorted by (work, fan_ix), a
        device-resident unit map of the script's words and device-resident side bytes, one per
        work: 0 out, 1 side A, 2 side B (fs_contrast_rows): per unit its works on either side,
        its statistic and in how many relabellings it, and the largest statistic of any unit,
        is reached; per permutation that largest statistic.  Without `out_ptrs`:
        (abi.CONTRAST_UNIT_DTYPE[n_units], abi.CONTRAST_PERM_DTYPE[permutations]) on the host.
        With `out_ptrs` = device addresses (units, permutations): they are written and () comes
        back.  Buffers torch has only just produced go in after torch_ready()."""
        L = _lib.load()

        def call(fixed, grown, caps, counts):
            return L.fs_contrast_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                      C.c_void_p(unit_of_ptr), int(n_units), int(min_words),
                                      int(max_gap), C.c_void_p(side_ptr), int(min_quoting),
                                      int(permutations), int(seed), int(key_bits),
                                      C.c_void_p(fixed[0]), C.c_void_p(fixed[1]))
        return _rows_call("fs_contrast_rows", call,
                          [(n_units, abi.CONTRAST_UNIT_DTYPE),
                           (permutations, abi.CONTRAST_PERM_DTYPE)], [], [], out_ptrs, "")

    def trends_device(self, rows_ptr, n_rows, n_works, unit_of_ptr, n_units, when_ptr,
                      min_words=6, max_gap=0, min_quoting=5, permutations=1000, seed=0,
                      out_ptrs=None):
        """`trends` over device-resident fs_row records sorted by (work, fan_ix), a
        device-resident unit map of the script's words and device-resident period offsets, 16
        bits per work: x(w) below 1024, or 0xFFFF for a work outside the pool (fs_trends_rows):
        per unit the works quoting it, the sum of their offsets, its statistic and in how many
        re-datings it, and the largest statistic of any unit, is reached; per re-dating the sum
        of the pool's offsets and that largest statistic.  Without `out_ptrs`:
        (abi.TRENDS_UNIT_DTYPE[n_units], abi.TRENDS_PERM_DTYPE[permutations]) on the host.
        With `out_ptrs` = device addresses (units, re-datings): they are written and () comes
        back.  Buffers torch has only just produced go in after torch_ready()."""
        L = _lib.load()

        def call(fixed, grown, caps, counts):
            return L.fs_trends_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                    C.c_void_p(unit_of_ptr), int(n_units), int(min_words),
                                    int(max_gap), C.c_void_p(when_ptr), int(min_quoting),
                                    int(permutations), int(seed), C.c_void_p(fixed[0]),
                                    C.c_void_p(fixed[1]))
        return _rows_call("fs_trends_rows", call,
                          [(n_units, abi.TRENDS_UNIT_DTYPE),
                           (permutations, abi.TRENDS_PERM_DTYPE)], [], [], out_ptrs, "")

    def neighbours_device(self, rows_ptr, n_rows, n_works, min_words=6, max_gap=0, weight=0,
                          top=10, min_score=1, min_similarity=0, out_ptrs=None, cap=None):
        """`neighbours` over device-resident fs_row records sorted by (work, fan_ix) (after a
        search or a gather; fs_neighbours_rows): per work its coverage, own score, candidates
        and how its list and the others' hold each other, per script word its depth and weight
        (`weight`: abi.FS_NEIGHBOURS_RARITY or abi.FS_NEIGHBOURS_FLAT), and every work's `top`
        closest works in (work, rank) order.  Without `out_ptrs`:
        (abi.NEIGHBOUR_WORK_DTYPE[n_works], abi.NEIGHBOUR_WORD_DTYPE[n_script],
        abi.NEIGHBOUR_DTYPE[n_listed]) on the host.  With `out_ptrs` = device addresses (works;
        words; listed pairs, a buffer of `cap` of them): the number of listed pairs;
        FsError(FS_E_CAPACITY) with .required when that buffer is too small (works and words
        are complete then).  Buffers torch has only just produced go in after torch_ready()."""
        L = _lib.load()
        n_script = int(self.info["n_script"])

        def call(fixed, grown, caps, counts):
            return L.fs_neighbours_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                        int(min_words), int(max_gap), int(weight), int(top),
                                        int(min_score), int(min_similarity), C.c_void_p(fixed[0]),
                                        C.c_void_p(fixed[1]), C.c_void_p(grown[0]), int(caps[0]),
                                        C.byref(counts[0]))
        return _rows_call("fs_neighbours_rows", call,
                          [(n_works, abi.NEIGHBOUR_WORK_DTYPE),
                           (n_script, abi.NEIGHBOUR_WORD_DTYPE)], [abi.NEIGHBOUR_DTYPE],
                          [_first_cap(cap, out_ptrs, 4096)], out_ptrs,
                          "listed pair buffer too small")

    def saturation_device(self, rows_ptr, n_rows, n_works, unit_of_ptr, n_units, min_words=6,
                          max_gap=0, permutations=1000, points=100, seed=0, level=95,
                          first=False, out_ptrs=None):
        """`saturation` over device-resident fs_row records sorted by (work, fan_ix) and a
        device-resident unit map of the script's words (fs_saturation_rows): works(u), per point
        of the curve the order statistics of the units seen and of the works sampled over the
        orders, per order where it passes half, nine tenths and all of the quoted units, and the
        summary's counts; with `first` also first(r, u), [n_units][permutations].  Without
        `out_ptrs`: (uint32[n_units], abi.SATURATION_POINT_DTYPE[points],
        abi.SATURATION_PERM_DTYPE[permutations], abi.SATURATION_SUMMARY_DTYPE[1]) on the host,
        then the uint32 first times with `first`.  With `out_ptrs` = device addresses (works,
        points, permutations, summary and, with `first`, the first times): they are written and
        () comes back.  Buffers torch has only just produced go in after torch_ready()."""
        L = _lib.load()

        def call(fixed, grown, caps, counts):
            return L.fs_saturation_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                        C.c_void_p(unit_of_ptr), int(n_units), int(min_words),
                                        int(max_gap), int(permutations), int(points), int(seed),
                                        int(level), C.c_void_p(fixed[0]), C.c_void_p(fixed[1]),
                                        C.c_void_p(fixed[2]), C.c_void_p(fixed[3]),
                                        C.c_void_p(fixed[4]) if first else None)
        fixed = [(n_units, np.uint32), (points, abi.SATURATION_POINT_DTYPE),
                 (permutations, abi.SATURATION_PERM_DTYPE), (1, abi.SATURATION_SUMMARY_DTYPE)]
        if first:
            fixed.append((int(n_units) * int(permutations), np.uint32))
        return _rows_call("fs_saturation_rows", call, fixed, [], [], out_ptrs, "")

    def transitions_device(self, rows_ptr, n_rows, n_works, unit_of_ptr, n_units, min_words=6,
                           max_gap=0, within=abi.FS_NONE, min_steps=1, min_step_works=2,
                           min_share=0, out_ptrs=None, cap=None):
        """`transitions` over device-resident fs_row records sorted by (work, fan_ix) and a
        device-resident unit map of the script's words (fs_transitions_rows): per unit its
        passages, works, starts, ends, steps and best successor, and the kept cells (a, b) of
        steps from unit a to unit b, in (a, b) order.  Without `out_ptrs`:
        (abi.TRANSITION_UNIT_DTYPE[n_units], abi.TRANSITION_DTYPE[n_cells]) on the host.  With
        `out_ptrs` = device addresses (units; cells, a buffer of `cap` of them): the number of
        cells; FsError(FS_E_CAPACITY) with .required when that buffer is too small (the units
        are complete then).  Buffers torch has only just produced go in after torch_ready()."""
        L = _lib.load()

        def call(fixed, grown, caps, counts):
            return L.fs_transitions_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                         C.c_void_p(unit_of_ptr), int(n_units), int(min_words),
                                         int(max_gap), int(within), int(min_steps),
                                         int(min_step_works), int(min_share),
                                         C.c_void_p(fixed[0]), C.c_void_p(grown[0]), int(caps[0]),
                                         C.byref(counts[0]))
        return _rows_call("fs_transitions_rows", call, [(n_units, abi.TRANSITION_UNIT_DTYPE)],
                          [abi.TRANSITION_DTYPE], [_first_cap(cap, out_ptrs, 4096)], out_ptrs,
                          "cell buffer too small")

    def clusters_device(self, rows_ptr, n_rows, n_works, min_words=6, max_gap=0, min_shared=6,
                        min_jaccard=50, min_size=2, common_pct=50, out_ptrs=None, cap=None):
        """`clusters` over device-resident fs_row records sorted by (work, fan_ix) (after a
        search or a gather; fs_clusters_rows): per work its family, links and best partner, and
        the families of >= min_size works in ascending order of root.  Without `out_ptrs`:
        (abi.CLUSTER_WORK_DTYPE[n_works], abi.CLUSTER_DTYPE[n_clusters]) on the host.  With
        `out_ptrs` = device addresses (works; clusters, a buffer of `cap` of them): the number
        of families; FsError(FS_E_CAPACITY) with .required when that buffer is too small (the
        works are complete then).  Buffers torch has only just produced go in after
        torch_ready()."""
        L = _lib.load()

        def call(fixed, grown, caps, counts):
            return L.fs_clusters_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                      int(min_words), int(max_gap), int(min_shared),
                                      int(min_jaccard), int(min_size), int(common_pct),
                                      C.c_void_p(fixed[0]), C.c_void_p(grown[0]), int(caps[0]),
                                      C.byref(counts[0]))
        return _rows_call("fs_clusters_rows", call, [(n_works, abi.CLUSTER_WORK_DTYPE)],
                          [abi.CLUSTER_DTYPE], [_first_cap(cap, out_ptrs, 4096)], out_ptrs,
                          "cluster buffer too small")

    def tree_device(self, rows_ptr, n_rows, n_works, min_words=6, max_gap=0, measure='jaccard',
                    min_shared=6, min_level=0, out_ptrs=None, caps=None):
        """`tree` over device-resident fs_row records sorted by (work, fan_ix) (after a search
        or a gather; fs_tree_rows): per work its tree, first merge and leaf, the merges in merge
        order and the levels, the highest first.  Without `out_ptrs`:
        (abi.TREE_WORK_DTYPE[n_works], abi.TREE_MERGE_DTYPE[n_merges],
        abi.TREE_LEVEL_DTYPE[n_levels]) on the host.  With `out_ptrs` = device addresses (works;
        merges and levels, buffers of `caps` = (merges, levels) of them): (n_merges, n_levels);
        FsError(FS_E_CAPACITY) with the same in .required when either buffer is too small (the
        works are complete then).  Buffers torch has only just produced go in after
        torch_ready()."""
        from .tree import measure_code
        L = _lib.load()
        code = measure_code(measure)

        def call(fixed, grown, caps, counts):
            return L.fs_tree_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                  int(min_words), int(max_gap), code, int(min_shared),
                                  int(min_level), C.c_void_p(fixed[0]), C.c_void_p(grown[0]),
                                  int(caps[0]), C.byref(counts[0]), C.c_void_p(grown[1]),
                                  int(caps[1]), C.byref(counts[1]))
        if caps is None:
            caps = (0, 0) if out_ptrs is not None else (4096, 256)
        return _rows_call("fs_tree_rows", call, [(n_works, abi.TREE_WORK_DTYPE)],
                          [abi.TREE_MERGE_DTYPE, abi.TREE_LEVEL_DTYPE], list(caps), out_ptrs,
                          "merge or level buffer too small")

    def retellings_device(self, rows_ptr, n_rows, n_works, min_words=6, max_gap=0, out_ptrs=None,
                          cap=None):
        """`retellings` over device-resident fs_row records sorted by (work, fan_ix) (after a
        search or a gather; fs_retellings_rows): per work its chain, and every passage with its
        best, prev, depth and place in the chain.  Without `out_ptrs`:
        (abi.RETELLING_DTYPE[n_works], abi.RETELLING_PASSAGE_DTYPE[n_passages]) on the host.
        With `out_ptrs` = device addresses (works; passages, a buffer of `cap` of them): the
        number of passages; FsError(FS_E_CAPACITY) with .required when that buffer is too small
        (the works are complete then).  Buffers torch has only just produced go in after
        torch_ready()."""
        L = _lib.load()

        def call(fixed, grown, caps, counts):
            return L.fs_retellings_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                        int(min_words), int(max_gap), C.c_void_p(fixed[0]),
                                        C.c_void_p(grown[0]), int(caps[0]), C.byref(counts[0]))
        cap = _first_cap(cap, out_ptrs, int(n_rows) // max(1, int(min_words)))
        return _rows_call("fs_retellings_rows", call, [(n_works, abi.RETELLING_DTYPE)],
                          [abi.RETELLING_PASSAGE_DTYPE], [cap], out_ptrs,
                          "passage buffer too small")

    def alignments_device(self, rows_ptr, n_rows, min_words=6, reach=4, match=2, gap=1,
                          out_ptrs=None, caps=None):
        """`alignments` over device-resident fs_row records sorted by (work, fan_ix) (after a
        search or a gather; fs_alignments_rows): the kept alignments in root order and the
        record indices of their paths.  Without `out_ptrs`: (abi.ALIGNMENT_DTYPE alignments,
        uint32 path records) on the host.  With `out_ptrs` = device addresses (alignments, a
        buffer of caps[0]; path records, a buffer of caps[1]): (alignments, path records)
        written; FsError(FS_E_CAPACITY) with .required = both counts when a buffer is too small
        (nothing is written then).  Buffers torch has only just produced go in after
        torch_ready()."""
        L = _lib.load()

        def call(_, grown, caps, counts):
            return L.fs_alignments_rows(self._h, C.c_void_p(rows_ptr), int(n_rows),
                                        int(min_words), int(reach), int(match), int(gap),
                                        C.c_void_p(grown[0]), int(caps[0]), C.byref(counts[0]),
                                        C.c_void_p(grown[1]), int(caps[1]), C.byref(counts[1]))
        caps = caps or ((0, 0) if out_ptrs is not None else
                        (min(int(n_rows) // max(1, int(min_words)), 4096),
                         min(int(n_rows), 1 << 16)))
        return _rows_call("fs_alignments_rows", call, [], [abi.ALIGNMENT_DTYPE, np.uint32], caps,
                          out_ptrs, "alignment or path buffer too small")

    def matrix_device(self, rows_ptr, n_rows, n_works, n_script, ngram=6, out_ptrs=None,
                      cap=None):
        """The n-grams of `matrix` over device-resident fs_row records sorted by
        (work, fan_ix) (after a search or a gather; fs_matrix_rows).  Without `out_ptrs`:
        (starts[n_script], n_spans, abi.MATRIX_NGRAM_DTYPE kept n-grams) on the host.  With
        `out_ptrs` = device addresses (starts, or 0 for none; n-grams, a buffer of `cap` of
        them): (n_spans, n_kept); FsError(FS_E_CAPACITY) with .required when that buffer is too
        small (starts is complete then).  Buffers torch has only just produced go in after
        torch_ready()."""
        L = _lib.load()
        spans = C.c_uint64(0)

        def call(fixed, grown, caps, counts):
            return L.fs_matrix_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                    int(n_script), int(ngram), C.c_void_p(fixed[0]),
                                    C.c_void_p(grown[0]), int(caps[0]), C.byref(spans),
                                    C.byref(counts[0]))
        cap = _first_cap(cap, out_ptrs, int(n_rows) // max(1, int(ngram)) + 1)
        got = _rows_call("fs_matrix_rows", call, [(n_script, np.uint32)],
                         [abi.MATRIX_NGRAM_DTYPE], [cap], out_ptrs, "n-gram buffer too small")
        if out_ptrs is not None:
            return int(spans.value), got
        return got[0], int(spans.value), got[1]

    def groups_device(self, rows_ptr, n_rows, n_works, mem_off, mem_grp, n_groups, label_of=None,
                      n_labels=0, min_words=6, max_gap=0, min_works=1, out_ptrs=None, caps=None):
        """`groups` over device-resident fs_row records sorted by (work, fan_ix) (after a search
        or a gather; fs_groups_rows); membership (mem_off, mem_grp) and label_of are host
        arrays.  Without `out_ptrs`: (abi.GROUP_DTYPE[n_groups], abi.GROUP_CELL_DTYPE cells,
        abi.GROUP_WORD_DTYPE rows) on the host.  With `out_ptrs` = device addresses (groups;
        cells, a buffer of caps[0]; word rows, a buffer of caps[1]): (cells, word rows) written;
        FsError(FS_E_CAPACITY) with .required = both counts when a buffer is too small (the
        groups are complete then).  Buffers torch has only just produced go in after
        torch_ready()."""
        L = _lib.load()
        mem_off, mem_grp = abi.as_u64(mem_off), abi.as_u32(mem_grp)
        lab = abi.as_u32(label_of) if n_labels else None

        def call(fixed, grown, caps, counts):
            return L.fs_groups_rows(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_works),
                                    abi.ptr(mem_off, C.c_uint64), abi.ptr(mem_grp, C.c_uint32),
                                    int(n_groups), abi.ptr(lab, C.c_uint32), int(n_labels),
                                    int(min_words), int(max_gap), int(min_works),
                                    C.c_void_p(fixed[0]), C.c_void_p(grown[0]), int(caps[0]),
                                    C.byref(counts[0]), C.c_void_p(grown[1]), int(caps[1]),
                                    C.byref(counts[1]))
        caps = caps or ((0, 0) if out_ptrs is not None else (4096, 1 << 16))
        return _rows_call("fs_groups_rows", call, [(n_groups, abi.GROUP_DTYPE)],
                          [abi.GROUP_CELL_DTYPE, abi.GROUP_WORD_DTYPE], caps, out_ptrs,
                          "cell or word buffer too small")

    def scan_benchmark(self, corpus, reps=20):
        """Average milliseconds of one scan-kernel launch over `corpus`."""
        ms = C.c_double(0)
        _lib.check(_lib.load().fs_scan_benchmark(self._h, corpus._h, reps, C.byref(ms)),
                   "fs_scan_benchmark")
        return ms.value

    def close(self):
        """Destroys the index; corpora created on it are closed first (the library
        would only detach them)."""
        for c in list(getattr(self, "_corpora", ())):
            c.close()
        if self._h:
            _lib.load().fs_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _fanon_canon(canon, canon_off):
    """The scripts' ids and offsets as the library takes them: none is one empty list."""
    if canon_off is None or len(canon_off) < 2:
        return np.zeros(1, np.uint32), np.zeros(1, np.uint64), 0
    off = abi.as_u64(canon_off)
    ids = abi.as_u32(canon)
    if len(ids) == 0:
        ids = np.zeros(1, np.uint32)
    return ids, off, len(off) - 1


def fanon(tok, work_off, n_ids, canon=None, canon_off=None, length=8, min_works=2,
          max_share=100, device=0):
    """`fanon` over host buffers (fs_fanon), which needs no script index: the token ids of the
    works `work_off` delimits, the scripts' ids (abi.FS_FANON_NO_ID for a word that is no fan
    token) under `canon_off`.  (works, shared grams in order of first, passages in corpus
    order, phrases in order of first, {'positions', 'distinct'}) as arrays of
    abi.FANON_*_DTYPE; the three growing buffers are enlarged until the call fits."""
    tok, off = abi.as_u32(tok), abi.as_u64(work_off)
    if len(off) < 1:
        raise ValueError("work_off needs at least its leading 0")
    n_works = len(off) - 1
    ids, coff, n_scripts = _fanon_canon(canon, canon_off)
    works = np.zeros(max(1, n_works), dtype=abi.FANON_WORK_DTYPE)
    n_pos, n_dist = C.c_uint64(0), C.c_uint64(0)
    L = _lib.load()
    from .command import grow
    grams, passages, phrases = grow(
        lambda g, cap_g, got_g, p, cap_p, got_p, f, cap_f, got_f: L.fs_fanon(
            int(device), abi.ptr(tok if len(tok) else np.zeros(1, np.uint32), C.c_uint32),
            abi.ptr(off, C.c_uint64), n_works, int(n_ids), abi.ptr(ids, C.c_uint32),
            abi.ptr(coff, C.c_uint64), n_scripts, int(length), int(min_works), int(max_share),
            works.ctypes.data_as(C.c_void_p), g, cap_g, p, cap_p, f, cap_f, got_g, got_p, got_f,
            C.byref(n_pos), C.byref(n_dist)),
        [abi.FANON_GRAM_DTYPE, abi.FANON_PASSAGE_DTYPE, abi.FANON_PHRASE_DTYPE],
        [1024, 1024, 1024], "fs_fanon")
    return works[:n_works], grams, passages, phrases, {'positions': int(n_pos.value),
                                                       'distinct': int(n_dist.value)}


def fanon_device(tok_ptr, n_tok, work_off_ptr, n_works, n_ids, canon_ptr=0, n_canon=0,
                 canon_off_ptr=0, n_scripts=0, length=8, min_works=2, max_share=100, device=0,
                 out_ptrs=None, caps=None, totals=None):
    """`fanon` over device-resident ids and offsets (fs_fanon_dev).  Without `out_ptrs`: (works,
    grams, passages, phrases) as host arrays, from buffers of torch's that grow until the call
    fits.  With `out_ptrs` = device addresses (works, grams, passages, phrases; the last three
    of `caps` records): (grams, passages, phrases) as counts; FsError(FS_E_CAPACITY) with
    .required = the three counts when a buffer is too small.  `totals`, a dict, receives
    'positions' and 'distinct'."""
    L = _lib.load()
    n_pos, n_dist = C.c_uint64(0), C.c_uint64(0)

    def call(fixed, grown, caps, counts):
        rc = L.fs_fanon_dev(int(device), C.c_void_p(tok_ptr), int(n_tok),
                            C.c_void_p(work_off_ptr), int(n_works), int(n_ids),
                            C.c_void_p(canon_ptr or None), int(n_canon),
                            C.c_void_p(canon_off_ptr or None), int(n_scripts), int(length),
                            int(min_works), int(max_share), C.c_void_p(fixed[0]),
                            C.c_void_p(grown[0]), int(caps[0]), C.c_void_p(grown[1]),
                            int(caps[1]), C.c_void_p(grown[2]), int(caps[2]),
                            C.byref(counts[0]), C.byref(counts[1]), C.byref(counts[2]),
                            C.byref(n_pos), C.byref(n_dist))
        if totals is not None:
            totals['positions'], totals['distinct'] = int(n_pos.value), int(n_dist.value)
        return rc
    caps = [int(c) for c in caps] if caps is not None else [0 if out_ptrs is not None else 1024] * 3
    return _rows_call("fs_fanon_dev", call, [(n_works, abi.FANON_WORK_DTYPE)],
                      [abi.FANON_GRAM_DTYPE, abi.FANON_PASSAGE_DTYPE, abi.FANON_PHRASE_DTYPE],
                      caps, out_ptrs, "gram, passage or phrase buffer too small")
