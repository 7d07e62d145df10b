"""The two branches every `*_device` method of ScriptIndex that takes a `cap` has, on the
smallest committed input of its command: with buffers of its own and room for one item it
repeats the call and returns what the default call returns; with the caller's buffers and room
for one item it raises FsError(FS_E_CAPACITY) whose .required is the true count, the fixed
output already complete.  (The tests of the commands make the second point with room for all
but one item of a large input, and check the results against the oracles.)"""

import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, companions, groups, synth
from fandom_search_amd.command import n_script_of, work_names
from fandom_search_amd.passages import read_matches, sort_records
from fandom_search_amd.quotes import word_labels
from fandom_search_amd.works import groups_of_labels
from tests.golden import make_groups_golden as mgg

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_SCRIPT = 1000          # of the index behind the fs_*_rows entry points: past every input's words


@pytest.fixture(scope="module")
def index(synth_base):
    from fandom_search_amd.engine import ScriptIndex
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [synth_base["words"][int(t)] for t in script], synth_base["emb"],
                     synth.lsh_normals(6))
    yield ix
    ix.close()


class Input:
    """A committed match CSV as the commands take it: sorted columns, and its records in HBM."""

    def __init__(self, name):
        import torch
        self.rows = read_matches(os.path.join(GOLDEN, name))
        _, self.work, self.fan, self.orig, dist, self.comb = sort_records(self.rows)
        self.names = work_names(self.rows)
        self.labels = word_labels(self.rows)
        assert n_script_of(self.orig) <= N_SCRIPT
        recs = np.zeros(len(self.work), dtype=abi.ROW_DTYPE)
        for field, col in (("work", self.work), ("fan_ix", self.fan), ("orig_ix", self.orig),
                           ("dist", dist), ("comb", self.comb)):
            recs[field] = col
        self.d_rows = torch.from_numpy(recs.view(np.uint8)).to("cuda")

    def scene_units(self):
        """(device unit map over the index's script, n_units) of --by scene."""
        import torch
        unit_of, about = companions.units_of(self.labels, self.work, self.fan, self.orig,
                                             self.comb, len(self.names), N_SCRIPT, "scene", 6, 0,
                                             1, 0)
        return torch.from_numpy(np.ascontiguousarray(unit_of, dtype=np.uint32)).to("cuda"), len(about)


def pairs_case(ix):
    f = Input("synthetic_n4.literal.csv")
    return [abi.PAIR_WORK_DTYPE, abi.PAIR_DTYPE], lambda **kw: ix.pairs_device(
        f.d_rows.data_ptr(), len(f.work), len(f.names), 4, 0, 1, **kw)


def clusters_case(ix):
    f = Input("synthetic_n4.literal.csv")
    return [abi.CLUSTER_WORK_DTYPE, abi.CLUSTER_DTYPE], lambda **kw: ix.clusters_device(
        f.d_rows.data_ptr(), len(f.work), len(f.names), 4, 0, 6, 50, 1, 50, **kw)


def companions_case(ix):
    f = Input("companions_lines.in.csv")
    d_map, n_units = f.scene_units()
    return [abi.COMPANION_UNIT_DTYPE, abi.COMPANION_DTYPE], \
        lambda **kw: ix.companions_device(f.d_rows.data_ptr(), len(f.work), len(f.names),
                                          d_map.data_ptr(), n_units, 6, 0, 2, 0, **kw)


def transitions_case(ix):
    f = Input("transitions_lines.in.csv")
    d_map, n_units = f.scene_units()
    return [abi.TRANSITION_UNIT_DTYPE, abi.TRANSITION_DTYPE], \
        lambda **kw: ix.transitions_device(f.d_rows.data_ptr(), len(f.work), len(f.names),
                                           d_map.data_ptr(), n_units, 6, 0, **kw)


def retellings_case(ix):
    f = Input("retellings_works.in.csv")
    return [abi.RETELLING_DTYPE, abi.RETELLING_PASSAGE_DTYPE], \
        lambda **kw: ix.retellings_device(f.d_rows.data_ptr(), len(f.work), len(f.names), 6, 0,
                                          **kw)


CASES = {"pairs": pairs_case, "clusters": clusters_case, "companions": companions_case,
         "transitions": transitions_case, "retellings": retellings_case}


def same(got, want):
    assert got.dtype == want.dtype and len(got) == len(want)
    for field in want.dtype.names or [None]:
        a, b = (got, want) if field is None else (got[field], want[field])
        assert np.array_equal(a, b), field


def device_buffers(counts, dtypes):
    """Zeroed device buffers of counts[k] records of dtypes[k], complete before a call."""
    import torch
    from fandom_search_amd.engine import torch_ready
    bufs = [torch.zeros(max(1, n) * np.dtype(d).itemsize, dtype=torch.uint8, device="cuda")
            for n, d in zip(counts, dtypes)]
    torch_ready()
    return bufs


def host_of(buf, n, dtype):
    return buf[:n * np.dtype(dtype).itemsize].cpu().numpy().view(dtype)


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_fixed_and_one_growing_output(name, index):
    from fandom_search_amd.engine import torch_ready
    dtypes, call = CASES[name](index)
    torch_ready()
    fixed, found = call()
    assert len(found) >= 2                                  # (else nothing below is tried)
    again = call(cap=1)
    same(again[0], fixed)
    same(again[1], found)
    bufs = device_buffers((len(fixed), 1), dtypes)
    with pytest.raises(_lib.FsError) as e:
        call(out_ptrs=[b.data_ptr() for b in bufs], cap=1)
    assert e.value.code == abi.FS_E_CAPACITY and e.value.required == len(found)
    same(host_of(bufs[0], len(fixed), dtypes[0]), fixed)    # the fixed output is complete


def test_matrix(index):
    from fandom_search_amd.engine import torch_ready
    f = Input("matrix_synthetic_n4.in.csv")
    n_script = n_script_of(f.orig)

    def call(**kw):
        return index.matrix_device(f.d_rows.data_ptr(), len(f.work), len(f.names), n_script, 4,
                                   **kw)
    torch_ready()
    starts, n_spans, kept = call()
    assert len(kept) >= 2 and n_spans >= len(kept)
    again = call(cap=1)
    same(again[0], starts)
    assert again[1] == n_spans
    same(again[2], kept)
    bufs = device_buffers((n_script, 1), (np.uint32, abi.MATRIX_NGRAM_DTYPE))
    with pytest.raises(_lib.FsError) as e:
        call(out_ptrs=[b.data_ptr() for b in bufs], cap=1)
    assert e.value.code == abi.FS_E_CAPACITY and e.value.required == len(kept)
    same(host_of(bufs[0], n_script, np.uint32), starts)     # starts is complete


def test_groups(index):
    from fandom_search_amd.engine import torch_ready
    f = Input("synthetic_n4.literal.csv")
    meta = groups.read_meta(os.path.join(GOLDEN, mgg.META), "year")
    keys, mem_off, mem_grp, _ = groups.membership(f.names, meta, "year")
    scene_of, scenes = groups_of_labels({o: lab[2] for o, lab in f.labels.items()}, N_SCRIPT)

    def call(**kw):
        return index.groups_device(f.d_rows.data_ptr(), len(f.work), len(f.names), mem_off,
                                   mem_grp, len(keys), scene_of, len(scenes), 4, 0, 1, **kw)
    torch_ready()
    found, cells, words = call()
    assert len(cells) >= 2 and len(words) >= 2
    dtypes = (abi.GROUP_DTYPE, abi.GROUP_CELL_DTYPE, abi.GROUP_WORD_DTYPE)
    for caps in ((1, 1), (1, len(words)), (len(cells), 1)):  # both short, then either
        for got, want in zip(call(caps=caps), (found, cells, words)):
            same(got, want)
        bufs = device_buffers((len(keys),) + caps, dtypes)
        with pytest.raises(_lib.FsError) as e:
            call(out_ptrs=[b.data_ptr() for b in bufs], caps=caps)
        assert e.value.code == abi.FS_E_CAPACITY
        assert e.value.required == (len(cells), len(words))
        same(host_of(bufs[0], len(keys), dtypes[0]), found)  # the groups are complete
