"""Given alignments at the aligner's prices on the CPU oracle (tests/given_ref.py): the restatement of include/svx.h's
svx_score_alignments is pinned to the oracle's own DP here, and the GPU entry is held to it in tests/test_gpu_given.py."""
import ctypes
import os

import numpy as np
import pytest

import given_ref
from around_ref import block_deletion_pair, true_pairs_found
from contact_ref import end_csum, widen_chain
from dp_ref import straight_stack
from synth import alignment_types, make_pair

TYPES5 = alignment_types(5)
FULL = os.path.join(os.path.dirname(__file__), "golden", "example_full")


@pytest.fixture(scope="module")
def clean(orc):
    """make_pair(200, 190, ..., deletions=3) through the straight band W = 7 -> (v0, v1, stack entry, its own path scored)."""
    v0, v1 = make_pair(200, 190, 4, 32, 5, deletions=3)
    st = straight_stack(orc, v0, v1, TYPES5, 7, 11)
    return v0, v1, st, given_ref.score(st, v0, v1, st['final_alignments'])


# ---------------------------------------------------------------------------------------------- 1
def test_own_path_costs_what_the_dp_added(clean):
    v0, v1, st, own = clean
    rows = len(st['final_alignments'])
    dels = sum(1 for x, y in st['final_alignments'] if not x or not y)
    assert dels > 0 and own['report'] == (rows, rows - dels, dels, 0, 0, 0, 0, 1)
    total = end_csum(st)
    assert np.abs(own['scores'] - st['alignment_scores']).max() <= 4 * 2.0 ** -52 * total
    assert abs(own['total'] - total) <= rows * 2.0 ** -52 * total
    assert own['del_penalty'] == st['del_penalty']


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("seed, want_outside, want_found", [(0, (206, 99, 0), (55, 126, 174)), (1, (206, 84, 0), (55, 134, 171))])
def test_block_deletion_table(orc, seed, want_outside, want_found):
    """rounds 0 and 1 of the doubling chain are search errors, round 2 is a model error."""
    v0, v1, src = block_deletion_pair(seed=seed)
    stacks, _ = widen_chain(orc, v0, v1, TYPES5, 7, 11)
    truth = given_ref.truth_path(src, 300)
    assert len(truth) == 300
    got = [given_ref.score(st, v0, v1, truth) for st in stacks]
    assert [st['a_b_csum'].shape[1] for st in stacks] == [14, 28, 56]
    assert tuple(g['report'][6] for g in got) == want_outside
    assert all(g['report'] == (300, 180, 120, 0, 0, 0, g['report'][6], 1) for g in got)
    assert tuple(true_pairs_found(st['final_alignments'], src) for st in stacks) == want_found
    found = [end_csum(st) for st in stacks]
    assert got[0]['total'] == got[1]['total'] == got[2]['total']       # same normalisers and penalty in every round
    assert got[0]['total'] < found[0] - 20 and got[1]['total'] < found[1] - 10 and found[2] < got[2]['total'] - 1
    if seed == 0:
        assert [round(f, 3) for f in found] == [191.216, 142.688, 118.578] and round(got[0]['total'], 3) == 120.569


# ---------------------------------------------------------------------------------------------- 3
def test_example_gold_is_a_model_error_as_far_as_it_can_be_priced(orc):
    from svx.utils.file_utils import read_alignments
    from svx.vecalign.dp_utils import complete_alignments, search_error
    from svx.vecalign.vecalign import make_alignment_types
    from test_example_full import load_side
    v0, v1 = load_side("en", "src"), load_side("de", "tgt")
    np.random.seed(0)
    st = orc.vecalign(v0.copy(), v1.copy(), make_alignment_types(6), 0.2, 8, 300, 20000, 100)[0]
    gold = read_alignments(os.path.join(FULL, "gold.txt"))
    path = complete_alignments(gold, 237, 217)
    assert (len(gold), len(path)) == (145, 147)
    got = given_ref.score(st, v0, v1, path)
    assert got['report'] == (147, 133, 11, 3, 0, 2, 0, 1)
    found = end_csum(st)
    assert search_error(found, got['total'], got['report']) == "unpriced"
    priced = got['total']            # the 133 priced rows and the 11 deletions: what can be priced of the gold path
    assert priced > found + 5 and round(found, 2) == 103.63 and round(priced, 2) == 116.25


# ---------------------------------------------------------------------------------------------- 4
def edited_paths(clean, count):
    """`count` one-edit neighbours of the found path that stay inside the band, scored -> [(alignments, scored)]."""
    v0, v1, st, own = clean
    rng = np.random.RandomState(2019)
    out = []
    while len(out) < count:
        for al in given_ref.edits(st['final_alignments'], TYPES5, 64, rng):
            s = given_ref.score(st, v0, v1, al)
            if s['report'][6] == 0 and len(out) < count:
                assert s['report'][3:6] == (0, 0, 0) and s['report'][7] == 1
                out.append((al, s))
    return out


def test_no_neighbour_of_the_found_path_is_cheaper(clean):
    v0, v1, st, own = clean
    total = end_csum(st)
    diffs = []
    for al, s in edited_paths(clean, 300):
        diffs.append(s['total'] - total)
        assert s['total'] >= total - given_ref.tolerance(s, own), (s['report'], s['total'], total)
    assert max(diffs) > 0.1          # the edits do change the price


# ---------------------------------------------------------------------------------------------- 5
def test_complete_alignments():
    from svx.utils.file_utils import read_alignments
    from svx.vecalign.dp_utils import complete_alignments, given_rows_from_alignments
    gold = read_alignments(os.path.join(FULL, "gold.txt"))
    path = complete_alignments(gold, 237, 217)
    assert len(path) == 147 and [a for a in path if a[0] and a[1]] == [a for a in gold if a[0] and a[1]]
    assert sorted(i for x, _ in path for i in x) == list(range(237)) and sorted(j for _, y in path for j in y) == list(range(217))
    assert all(len(x) + len(y) == 1 for x, y in path if not x or not y)
    assert complete_alignments(path, 237, 217) == path                        # already complete
    rows = given_rows_from_alignments(path)
    assert (rows[1:, 0] == rows[:-1, 0] + rows[:-1, 1]).all() and (rows[1:, 2] == rows[:-1, 2] + rows[:-1, 3]).all()
    assert tuple(rows[-1, [0, 2]] + rows[-1, [1, 3]]) == (237, 217)
    # a one-sided line of several segments, gaps on both sides, a tail
    got = complete_alignments([([1, 2], [0]), ([4, 5, 6], []), ([7], [3])], 9, 4)
    assert got == [([0], []), ([1, 2], [0]), ([3], []), ([4], []), ([5], []), ([6], []), ([], [1]), ([], [2]), ([7], [3]), ([8], [])]
    assert complete_alignments([], 2, 1) == [([0], []), ([1], []), ([], [0])]
    with pytest.raises(ValueError, match="line 2.*contiguous"):
        complete_alignments([([0], [0]), ([1, 3], [1])], 5, 5)
    with pytest.raises(ValueError, match="line 2.*backwards"):
        complete_alignments([([0, 1], [0]), ([1], [1])], 5, 5)
    with pytest.raises(ValueError, match="line 1.*leaves"):
        complete_alignments([([0], [4, 5])], 5, 5)


def test_search_error_verdicts():
    from svx.vecalign.dp_utils import search_error
    ok = (10, 8, 2, 0, 0, 1, 3, 1)
    assert search_error(5.0, 4.999, ok) == "search" and search_error(5.0, 5.0, ok) == "model" and search_error(5.0, 6.0, ok) == "model"
    for bad in ((10, 8, 1, 1, 0, 0, 0, 1), (10, 8, 1, 0, 1, 0, 0, 0), (10, 8, 2, 0, 0, 0, 0, 0), (-1,) * 8):
        assert search_error(5.0, 1.0, bad) == "unpriced"


def test_poisoned_rows_are_classified_without_being_read(clean):
    v0, v1, st, own = clean
    rows = given_ref.rows_of(st['final_alignments'])
    bad = rows.copy()
    bad[3] = (-1, 1, 5, 1)
    bad[5] = (given_ref.INT32_MAX, given_ref.INT32_MAX, 0, 1)
    bad[7] = (bad[7][0], 0, bad[7][2], 0)
    bad[9] = (bad[9][0], 2, bad[9][2], 0)
    bad[11] = (bad[11][0], 5, bad[11][2], 1)
    got = given_ref.score(st, v0, v1, bad)
    assert got['report'][3:5] == (1, 4) and got['report'][7] == 0
    assert np.isnan(got['scores'][[3, 5, 7, 9, 11]]).all() and np.isfinite(np.delete(got['scores'], [3, 5, 7, 9, 11])).all()


def test_the_new_flags_parse():
    from svx.seg_align import align
    base = ["meta.txt", "out", "--src_lang", "en", "--tgt_lang", "de", "--seg_dir", "s", "--concat_dir", "c", "--embed_dir", "e"]
    a = align.parse_args(base)
    assert (a.rescore_dir, a.rescore_tsv) == (None, None)
    a = align.parse_args(base + ["--rescore_dir", "g", "--rescore_tsv", "g.tsv", "--mode", "band", "--band", "14"])
    assert (a.rescore_dir, a.rescore_tsv) == ("g", "g.tsv")
    assert str(align.rescore_path(a, align.VecalignData("", "", "", "", "", "", "o/en-de/x-y.txt"))) == os.path.join("g", "en-de", "x-y.txt")
    for extra in (["--rescore_dir", "g"], ["--rescore_tsv", "g.tsv"], ["--rescore_dir", "g", "--rescore_tsv", "g.tsv", "--widen"],
                  ["--rescore_dir", "g", "--rescore_tsv", "g.tsv", "--skip_existing"]):
        with pytest.raises(SystemExit):
            align.parse_args(base + extra)


def test_library_exports_the_entry():
    """Fails on a build without the feature, with no GPU."""
    from svx import _lib
    lib = _lib.load()
    assert hasattr(lib, "svx_score_alignments") and "svx_score_alignments" in _lib.EXPORTS
    assert ctypes.sizeof(_lib.Given) == 48
    assert [f[0] for f in _lib.Given._fields_] == ["rows", "info", "cap", "pad", "scores", "total", "report"]
