"""What a search launches, held to a recorded table: for every case of tools/plan_table.py (an
index recipe plus FS_* switches) the kernel name, the scan shape, the path, the scan launches, the
hand-off fallbacks and the number of rows must be what tests/golden/plan_table.json holds.

The golden file is the output of tools/plan_table.py on commit a7b7e09 ("Test the float32 LSH
key signs on cancelling sums; fix subnormal bound"), the last one that decided a search's
kernels in fs_search_corpus_begin, search_enqueue, fs_search_corpus_end, fs_search_kernel_name
and fs_index_scan_shape separately, run on an MI355X with every case in a process of its own.
The expected values are that commit's, never this tree's: the file is not to be regenerated from
the code under test."""

import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_tool():
    spec = importlib.util.spec_from_file_location("plan_table_tool", os.path.join(ROOT, "tools", "plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


plan_table = _load_tool()

with open(os.path.join(ROOT, "tests", "golden", "plan_table.json")) as _f:
    GOLDEN = {e["case"]: e for e in (json.loads(line) for line in _f if line.strip())}


def test_the_golden_file_holds_every_case_and_no_other():
    assert sorted(GOLDEN) == sorted(plan_table.CASES)


@pytest.mark.parametrize("case", sorted(plan_table.CASES))
def test_plan_equals_the_recorded_one(case):
    got = plan_table.run_case(case)
    print(json.dumps(got, sort_keys=True))
    assert got == GOLDEN[case]


def test_the_recorded_table_covers_every_path():
    """(of the golden file itself: the cases reach every kernel name the planner can give, the
    growth of each capacity and the hand-off's fallback)"""
    names = {e["kernel_name"] for e in GOLDEN.values()}
    assert names >= {"k_scan_rows<4,3>", "k_scan8<4>", "k_scan<4>", "k_scan<9>", "k_scan<12>", "k_near_sift<8>",
                     "k_scan_near8<8>", "k_scan_near<8>", "k_lsh_scan", "k_near_sift<6>", "k_scan_near<6>",
                     "k_share_scan<6>", ""}
    assert GOLDEN["exact4_wait_spins_0"]["handoff_fallbacks"] > 0 and GOLDEN["exact4_wait_spins_0"]["scan_launches"] == 2
    for grown in ("exact4_scan_capw_2", "exact4_ranges_caprow_2", "general8_scan_capw_2"):
        assert GOLDEN[grown]["scan_launches"] == 2
    assert GOLDEN["exact4_host_wire8_0"]["scan_shape"]["host_wire8"] == 0
    assert GOLDEN["exact4_lanes_4"]["scan_shape"]["waves"] == 8
