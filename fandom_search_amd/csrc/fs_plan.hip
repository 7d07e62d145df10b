// fs_plan.hip -- what a search launches (fs_plan, fs_internal.h), decided in one place.
// Host code only.  The table of paths in DESIGN.md section 6 is written from this function.
#include "fs_internal.h"

#include <stdio.h>

#include <algorithm>

fs_plan fs_plan_search(const fs_index* ix, const fs_corpus* c, int rows_mode, const fs_index::Lane& ln,
                       bool chained_only) {
  const fs_switches& sw = ix->sw;
  const uint64_t T = c->n_tok;
  const int n = (int)ix->cfg.window_size;
  fs_plan p;
  // out-of-vocabulary vectors are outside the exact n-gram proof: such a batch takes the general pipeline
  p.exact = ix->info.path == FS_MODE_EXACT && !c->has_oov;
  // (host rows of the exact pipeline leave the device as 8-byte records: a quarter of the bytes over PCIe)
  p.host_wire8 = rows_mode == FS_ROWS_HOST && p.exact && ix->n_script < (1ull << 18) && sw.host_wire8;
  p.ccap = std::max<uint64_t>(std::max<uint64_t>(4096, T / 16), ln.w_cpos.n);
  if (p.exact && !chained_only) p.waves = fs_scan_rows_shape(ix, c, &p.blocks);
  if (p.waves) {
    // k_scan_rows (tokens -> records in one kernel).  Staged records per wave range: a sixteenth of
    // its tokens (C2: 305, 72 used on average), more once a search has asked for it
    p.path = FS_PATH_ROWS;
    p.sub_k = sw.scan_sub && ix->d_sfilter.p ? fs_sub_k(n) : 0;
    p.tpl = 8;
    // the 16-bit copy of the ids where the batch has one (every id below 2^16) and no string ids
    // of its own (that instance keeps the 32-bit stream)
    p.ids16 = sw.scan_ids16 && c->tok16_ok && c->d_tok16.p && !c->has_str;
    const uint32_t ranges = p.blocks * p.waves;
    const uint32_t dflt = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(128, T / ranges / 16), 1u << 20);
    p.caprow = std::max<uint32_t>(dflt, ln.caprow_hint);
    if (sw.ranges_caprow > 0) p.caprow = (uint32_t)sw.ranges_caprow;
  } else if (p.exact || chained_only) {
    // the chained kernels.  Direct (the scan writes candidate records per wave range): 64 records
    // per range to start with (C2 needs about 20), more once a search has asked for it
    p.tpl = fs_scan_tpl(ix);
    p.path = fs_scan_direct_ok(ix, T) ? FS_PATH_DIRECT : FS_PATH_BITMAP;
    if (p.path == FS_PATH_DIRECT) {
      p.capw = std::max<uint32_t>(64, ln.capw_hint);
      if (sw.scan_capw > 0) p.capw = (uint32_t)sw.scan_capw;   // tests: force the growth path
    }
  } else if (fs_lsh_prefilter_mode(ix, c) == 0) {
    // no integer prefilter applies: keys and buckets for every window (four tokens per lane)
    p.path = FS_PATH_KEY_SCAN;
    p.share_scan = (ix->share_flags & 32) != 0;
  } else {
    // tables whose proof fails by one slot only: the integer prefilter flags the windows that can
    // have a neighbour at all (k_scan_near8 writes eight tokens per lane, k_scan_near four)
    p.near8 = ix->near8;
    p.tpl = p.near8 ? 8 : 4;
    p.path = p.near8 && sw.near_fused ? FS_PATH_NEAR_SIFT : FS_PATH_NEAR_CHAIN;
    if (p.path == FS_PATH_NEAR_SIFT) {
      // list entries per wave range: an eighth of its tokens to start with (a C2 batch uses 17 of
      // 305 on average at n = 8, 112 over component ids at n = 6), more once a search has asked for it
      p.caps = std::max<uint32_t>((uint32_t)std::min<uint64_t>(std::max<uint64_t>(64, T / fs_near_ranges() / 8), 1u << 20),
                                  ln.caps_hint);
      if (sw.scan_capw > 0) p.caps = (uint32_t)sw.scan_capw;   // tests: force the growth path
    }
  }
  p.n_bm = (uint32_t)((T + 64 * p.tpl - 1) / (64 * p.tpl));
  return p;
}

const char* fs_plan_kernel_name(const fs_index* ix, const fs_plan& p) {
  static thread_local char name[64];
  const int n = (int)ix->cfg.window_size;
  switch (p.path) {
    case FS_PATH_ROWS: snprintf(name, sizeof name, "k_scan_rows<%d,%d>", n, p.sub_k); break;
    case FS_PATH_DIRECT:
    case FS_PATH_BITMAP: snprintf(name, sizeof name, p.tpl == 8 ? "k_scan8<%d>" : "k_scan<%d>", n); break;
    case FS_PATH_NEAR_SIFT: snprintf(name, sizeof name, "k_near_sift<%d>", n); break;
    case FS_PATH_NEAR_CHAIN: snprintf(name, sizeof name, p.near8 ? "k_scan_near8<%d>" : "k_scan_near<%d>", n); break;
    case FS_PATH_KEY_SCAN: snprintf(name, sizeof name, p.share_scan ? "k_share_scan<%d>" : "k_lsh_scan", n); break;
  }
  return name;
}
