"""`ao3.py search fan_works script [script ...] [--out-dir DIR]` on the host: the parser's
shape, where each script's files go, and the refusals that come before any work is read and
before the HIP library is loaded."""

import datetime
import os
import subprocess
import sys

import pytest

from fandom_search_amd import search
from fandom_search_amd.cli import build_parser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parser_takes_several_scripts():
    a = build_parser().parse_args(["search", "fan", "s/a.txt", "t/b.txt", "c.txt", "-n", "5",
                                   "--out-dir", "out"])
    assert a.script == "s/a.txt"
    assert a.scripts == ["s/a.txt", "t/b.txt", "c.txt"]
    assert (a.fan_works, a.num_works, a.out_dir) == ("fan", 5, "out")
    a = build_parser().parse_args(["search", "fan", "one.txt"])
    assert (a.script, a.scripts, a.out_dir) == ("one.txt", ["one.txt"], None)


def test_output_directory_of_each_script():
    assert search.script_out_dirs(["scripts/sw-new-hope.txt"]) == [""]
    assert search.script_out_dirs(["scripts/sw-new-hope.txt"], "D") == ["D"]
    assert search.script_out_dirs(["scripts/sw-new-hope.txt", "x/sw-empire.txt"]) == \
        [os.path.join(".", "sw-new-hope"), os.path.join(".", "sw-empire")]
    assert search.script_out_dirs(["scripts/sw-new-hope.txt", "sw-empire"], "D") == \
        [os.path.join("D", "sw-new-hope"), os.path.join("D", "sw-empire")]
    with pytest.raises(ValueError):
        search.script_out_dirs(["a/sw.txt", "b/sw.txt"])
    with pytest.raises(ValueError):
        search.script_out_dirs(["sw.txt", "sw.txt"], "D")


def test_date_suffix_per_directory(tmp_path):
    today = "{:%Y%m%d}".format(datetime.date.today())
    for d in ("a", "b"):
        (tmp_path / d).mkdir()
    (tmp_path / "a" / ("match-6gram-%s.csv" % today)).write_text("x")
    base = "match-6gram{}"
    got_a = search.unused_result_name(os.path.join(str(tmp_path / "a"), base))
    got_b = search.unused_result_name(os.path.join(str(tmp_path / "b"), base))
    assert got_a == os.path.join(str(tmp_path / "a"), "match-6gram-%s-1.csv" % today)
    assert got_b == os.path.join(str(tmp_path / "b"), "match-6gram-%s.csv" % today)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from fandom_search_amd.cli import main
code = None
try:
    main(sys.argv[2:])
except SystemExit as e:
    code = e.code
maps = open("/proc/self/maps").read()
print("LIBRARY LOADED" if "libfandomsearch_hip" in maps else "LIBRARY NOT LOADED")
print("EXIT", code)
"""


def _child(args, env_extra, tmp_path):
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT] + args, env=env, cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    return r.stdout, r.stderr


@pytest.mark.parametrize("case", ["same stem", "same script", "launcher"])
def test_refused_before_the_library_loads(tmp_path, case):
    # (the fan-works directory does not exist: reading it would fail with another error)
    fan = str(tmp_path / "no-such-dir")
    env = {}
    if case == "same stem":
        scripts = ["one/sw.txt", "two/sw.txt"]
    elif case == "same script":
        scripts = ["sw.txt", "sw.txt"]
    else:
        scripts = ["sw-a.txt", "sw-b.txt"]
        env = {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"}
    out, err = _child(["search", fan] + scripts, env, tmp_path)
    assert "LIBRARY NOT LOADED" in out, (out, err)
    assert "EXIT ao3.py search: error:" in out or "error:" in err, (out, err)
    msg = out + err
    assert ("launcher" in msg) if case == "launcher" else ("file name of its own" in msg), msg
    assert not os.listdir(str(tmp_path))
