"""The band search around a prior alignment on the CPU oracle (tests/around_ref.py), and the host-only pieces of the
feature: what svx_align_around / svx_time_prior are held to on the GPU (tests/test_gpu_around.py)."""
import numpy as np
import pytest

from around_ref import (SVX_ERR_ARG, SVX_ERR_EXTEND, SVX_ERR_PATH, SVX_ERR_TRACEBACK, around_stack, block_deletion_pair,
                        block_prior, ingest_ref, lengths_to_alignments, time_prior_ref, true_pairs_found)
from dp_ref import straight_stack
from synth import alignment_types, make_pair


def test_refinement_around_the_dense_prior_is_the_level0_refinement(orc):
    """At max_depth == 0 the reference refines around its same-level dense 1-1 alignment (dp_utils.py:485-489): the
    search around that alignment as a prior is vecalign()'s own result, bit for bit."""
    v0, v1 = make_pair(120, 97, K=4, d=32, seed=3, deletions=6)
    types = alignment_types(5)
    np.random.seed(11)
    ref = orc.vecalign(v0.copy(), v1.copy(), types, 0.2, 7, 300, 20000, 100)
    assert len(ref) == 1   # L = 0
    got = around_stack(orc, v0, v1, types, 7, 11, ref[0]['alignments'])
    assert got['searchpath'] == [tuple(p) for p in ref[0]['searchpath']]
    assert got['final_alignments'] == ref[0]['final_alignments']
    assert np.array_equal(got['alignment_scores'], ref[0]['alignment_scores'])
    assert np.array_equal(got['b_offset'], ref[0]['b_offset'])


def test_block_prior_recovers_what_the_straight_band_cannot(orc):
    """300 source segments, the target lacks source segments 100..219 (M = 180), a = 5, W = 7.  A true pair (s, j) lies
    |j - 0.375 (s + j)| cells off the straight line: within the band's W + 1 only for the first and the last ~4 (W + 1)
    target segments, so the straight search can hold at most 8 (W + 1) = 64 of the 180 true pairs.  A prior of 15 blocks
    of 20 source segments with their target segments leaves every true pair inside a block; the search around it finds
    what the coarse-to-fine search finds.  (block_deletion_pair(seed=0): 55, 174 and 174 of 180.)"""
    v0, v1, src = block_deletion_pair(seed=0)
    types = alignment_types(5)
    assert v1.shape[1] == 180
    straight = straight_stack(orc, v0, v1, types, 7, 11)
    prior = block_prior(src, 300)
    assert len(prior) == 15
    around = around_stack(orc, v0, v1, types, 7, 11, prior)
    c2f = orc.vecalign(v0.copy(), v1.copy(), types, 0.2, 7, 100, 20000, 100, rng=np.random.RandomState(11))
    n_straight = true_pairs_found(straight['final_alignments'], src)
    n_around = true_pairs_found(around['final_alignments'], src)
    n_c2f = true_pairs_found(c2f[0]['final_alignments'], src)
    print("true pairs found: straight %d, around %d, coarse-to-fine %d of 180" % (n_straight, n_around, n_c2f))
    assert n_straight <= 64
    assert n_around >= 162 and n_around == n_c2f


def test_single_block_prior_is_the_straight_search(orc):
    v0, v1 = make_pair(200, 190, 4, 32, seed=5, deletions=3)
    types = alignment_types(5)
    a = straight_stack(orc, v0, v1, types, 16, 21)
    b = around_stack(orc, v0, v1, types, 16, 21, [(list(range(200)), list(range(190)))])
    for k in ('a_b_costs', 'b_offset', 'a_b_csum', 'a_b_xp', 'a_b_yp', 'new_b_offset', 'alignment_scores'):
        assert np.array_equal(a[k], b[k]), k
    assert a['final_alignments'] == b['final_alignments']
    # count = 0: the ingest appends the remainder (n, m), which is that block
    lengths, code = ingest_ref(np.zeros((0, 4)), 0, 200, 190)
    assert code == 0 and lengths_to_alignments(lengths) == [(list(range(200)), list(range(190)))]


def test_ingest_rules():
    rows = np.array([[0, 2, 0, 1], [2, 0, 1, 3], [2, 4, 4, 0]])
    lengths, code = ingest_ref(rows, 3, 10, 6)
    assert code == 0 and lengths.tolist() == [[2, 1], [0, 3], [4, 0], [4, 2]]
    lengths, code = ingest_ref(rows, 3, 6, 6)
    assert code == 0 and lengths.tolist() == [[2, 1], [0, 3], [4, 0], [0, 2]]     # a deletion run as remainder
    lengths, code = ingest_ref(rows, 3, 6, 4)
    assert code == 0 and lengths.tolist() == [[2, 1], [0, 3], [4, 0]]             # exact: nothing appended
    assert ingest_ref(rows, 3, 5, 6)[1] == SVX_ERR_EXTEND
    assert ingest_ref(rows, 3, 10, 3)[1] == SVX_ERR_EXTEND
    assert ingest_ref(rows, 4, 10, 6)[1] == SVX_ERR_ARG and ingest_ref(rows, -1, 10, 6)[1] == SVX_ERR_ARG
    assert ingest_ref(rows, 3, 10, 6, code=SVX_ERR_TRACEBACK)[1] == SVX_ERR_TRACEBACK
    assert ingest_ref([[0, 1, 0, 1], [1, 0, 1, 0]], 2, 9, 9)[1] == SVX_ERR_PATH
    assert ingest_ref([[0, 1, 0, 1], [1, -1, 1, 5]], 2, 9, 9)[1] == SVX_ERR_PATH  # (before the sums are looked at)
    assert ingest_ref(rows, 2, 10, 6)[0].tolist() == [[2, 1], [0, 3], [8, 2]]     # rows past count are not read


def test_time_prior_hand_written():
    """6 x 5 segments, window 100, lag -30 (the target runs AHEAD: its starts are moved 30 later).  Source windows
    0 0 1 1 3 3 (a start exactly on the edge 100 opens window 1; window 2 is empty on both sides); target starts
    0 60 70 200 370 -> shifted 30 90 100 230 400 -> windows 0 0 1 2 4: window 2 on the target only, 3 on the source only, 4
    on the target only, at the end."""
    F0 = [(0, 10), (99, 100), (100, 150), (199, 220), (300, 310), (399, 420)]
    F1 = [(0, 5), (60, 65), (70, 90), (200, 210), (370, 380)]
    rows, code = time_prior_ref(F0, F1, 100, -30)
    assert code == 0
    assert rows.tolist() == [[0, 2, 0, 2], [2, 2, 2, 1], [4, 0, 3, 1], [4, 2, 4, 0], [6, 0, 4, 1]]
    assert rows[:, 1].sum() == 6 and rows[:, 3].sum() == 5
    # a positive lag larger than the first starts clamps at 0 instead of opening negative windows
    rows, code = time_prior_ref(F0, F1, 100, 65)
    assert code == 0 and rows.tolist() == [[0, 2, 0, 3], [2, 2, 3, 1], [4, 2, 4, 1]]
    assert time_prior_ref(F0, [(5, 6), (4, 9)], 100, 0)[1] == SVX_ERR_PATH
    assert time_prior_ref(F0, [(5, 6), (5, 9)], 100, 0)[1] == 0                   # equal starts do not decrease


def test_prior_rows_from_alignments():
    from svx.vecalign.dp_utils import prior_rows_from_alignments
    al = [([0], [0]), ([], [1, 2]), ([1, 2, 3], [3, 4]), ([4], []), ([5, 6], [5, 6, 7, 8])]
    rows = prior_rows_from_alignments(al)
    assert rows.dtype == np.int32 and rows.shape == (5, 4)
    assert rows.tolist() == [[0, 1, 0, 1], [1, 0, 1, 2], [1, 3, 3, 2], [4, 1, 5, 0], [5, 2, 5, 4]]
    # the ids are not read: lengths from len(), starts running
    assert prior_rows_from_alignments([([7, 9], [3]), ([], [0])]).tolist() == [[0, 2, 0, 1], [2, 0, 1, 1]]
    empty = prior_rows_from_alignments([])
    assert empty.shape == (0, 4) and empty.dtype == np.int32
    lengths, code = ingest_ref(rows, len(rows), 7, 9)
    assert code == 0 and lengths_to_alignments(lengths) == al


def test_cli_needs_exactly_one_prior():
    from svx.seg_align import align as A
    base = ["meta.tsv", "out", "--src_lang", "en", "--tgt_lang", "de", "--seg_dir", "s", "--concat_dir", "c", "--embed_dir", "e", "--mode", "around"]
    for extra in ([], ["--prior_dir", "p", "--prior", "time"]):
        with pytest.raises(SystemExit):
            A.parse_args(base + extra)
    assert A.parse_args(base + ["--prior", "time"]).prior_window == 30.0
