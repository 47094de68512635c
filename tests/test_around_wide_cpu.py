"""Wide bands around a prior (include/svx.h: SVX_SEARCH_AROUND_WIDE, svx_prior_width) on the CPU oracle: the covering
property svx_prior_width is documented with, its host twin, what a covering band recovers, and the CLI's --prior_band."""
import numpy as np
import pytest

from around_ref import around_stack, block_deletion_pair, block_prior, ingest_ref, lengths_to_alignments, true_pairs_found
from synth import alignment_types

N, M = 300, 180
STEPS = (20, 60, 100, 150, 300)            # priors of 15, 5, 3, 2 blocks and 1 block
COVERING = {20: 21, 60: 61, 100: 101, 150: 101, 300: 181}


@pytest.fixture(scope="module")
def pair():
    return block_deletion_pair(seed=0)


def new_b_offset(orc, prior, n, m, W):
    """new_b_offset of sparse_dp around the prior's search path (dp_core.pyx: b_offset of the point two diagonals back, + 1)."""
    path = np.asarray(orc.search_path(prior, False, n, m)).reshape(-1, 2)
    assert len(path) == n + m + 1 and (path.sum(axis=1) == np.arange(n + m + 1)).all()   # one point per diagonal
    out = np.empty(len(path) + 2, np.int64)
    out[:2] = path[0, 1] - W
    out[2:] = path[:, 1] + 1 - W
    return out


def uncovered_nodes(nbo, lengths, W):
    """Nodes (x, y) of the blocks, ends included, outside the band 0 <= y - new_b_offset[x + y] < 2 W."""
    bad, x0, y0 = 0, 0, 0
    for xl, yl in np.asarray(lengths).tolist():
        xs, ys = np.meshgrid(np.arange(x0, x0 + xl + 1), np.arange(y0, y0 + yl + 1), indexing='ij')
        b = ys - nbo[xs + ys]
        bad += int(((b < 0) | (b >= 2 * W)).sum())
        x0, y0 = x0 + xl, y0 + yl
    return bad


def test_covering_property(orc, pair):
    from svx.vecalign.dp_utils import prior_rows_from_alignments, prior_width
    src = pair[2]
    priors = [block_prior(src, N, step) for step in STEPS]
    # deletion rows on either side, and sums below (n, m): the ingest appends the remainder (100, 50)
    rows = np.array([[0, 40, 0, 30], [40, 0, 30, 10], [40, 25, 40, 0], [65, 60, 40, 50], [125, 5, 90, 0], [130, 70, 90, 40]])
    lengths, code = ingest_ref(rows, len(rows), N, M)
    assert code == 0 and lengths[-1].tolist() == [100, 50]
    cases = [(prior_rows_from_alignments(p), p) for p in priors] + [(rows, lengths_to_alignments(lengths))]
    narrow_bad = []
    for r, full in cases:
        W = prior_width(r, N, M)
        ing, code = ingest_ref(r, len(r), N, M)
        assert code == 0 and W == max(3, 1 + int(ing.min(axis=1).max()))
        assert uncovered_nodes(new_b_offset(orc, full, N, M, W), ing, W) == 0
        narrow_bad.append(uncovered_nodes(new_b_offset(orc, full, N, M, 7), ing, 7))
    assert [prior_width(prior_rows_from_alignments(p), N, M) for p in priors] == [COVERING[s] for s in STEPS]
    assert min(narrow_bad[:5]) == 450 and max(narrow_bad[:5]) == 47941 and narrow_bad[5] > 0


def test_band_offsets_of_the_helper_are_the_oracles(orc, pair):
    v0, v1, src = pair
    prior = block_prior(src, N, 100)
    ref = around_stack(orc, v0, v1, [(1, 1)], 9, 11, prior)
    assert np.array_equal(new_b_offset(orc, prior, N, M, 9), ref['new_b_offset'])


def test_host_prior_width_hand_written():
    from svx.vecalign.dp_utils import prior_width
    rows = np.array([[0, 2, 0, 1], [2, 0, 1, 3], [2, 4, 4, 9], [6, 4, 13, 0]])
    assert prior_width(rows, 10, 13) == 5                       # max of min = 4 (row 2); no remainder
    assert prior_width(rows, 30, 40) == 21                      # remainder (20, 27)
    assert prior_width(rows, 30, 13) == 5                       # remainder (20, 0): a deletion run
    assert prior_width(rows[:2], 2, 4) == 3                     # never below 3
    assert prior_width(np.zeros((0, 4), np.int32), 200, 190) == 191 and prior_width([], 64, 1) == 3   # the straight search
    assert prior_width([([0, 1], [0]), ([], [1, 2, 3]), ([2, 3, 4, 5], list(range(4, 13)))], 6, 13) == 5   # alignments
    # priors the ingest fails: 0
    assert prior_width(rows, 9, 13) == 0 and prior_width(rows, 10, 12) == 0                       # SVX_ERR_EXTEND
    assert prior_width([[0, 1, 0, 1], [1, 0, 1, 0]], 9, 9) == 0 and prior_width([[0, -1, 0, 5]], 9, 9) == 0   # SVX_ERR_PATH


def test_a_covering_band_recovers_what_the_coarse_prior_loses(orc, pair):
    """True 1-1 pairs found of 180, -a 5, seed 11: every prior at its covering width finds what the coarse-to-fine
    search finds; at W = 7 a prior of 2 blocks is no better than the straight band (at most 8 (W + 1) = 64)."""
    from svx.vecalign.dp_utils import prior_rows_from_alignments, prior_width
    v0, v1, src = pair
    types = alignment_types(5)
    c2f = orc.vecalign(v0.copy(), v1.copy(), types, 0.2, 7, 100, 20000, 100, rng=np.random.RandomState(11))
    n_c2f = true_pairs_found(c2f[0]['final_alignments'], src)
    found = {}
    for step in STEPS:
        prior = block_prior(src, N, step)
        W = prior_width(prior_rows_from_alignments(prior), N, M)
        found[step] = tuple(true_pairs_found(around_stack(orc, v0, v1, types, w, 11, prior)['final_alignments'], src) for w in (7, W))
    print("true pairs found (W = 7, covering W) per block step:", found, "coarse-to-fine:", n_c2f)
    assert n_c2f == 174
    assert found[150][0] <= 64 and found[300][0] <= 64
    assert all(found[s][1] == n_c2f for s in STEPS)
    assert found == {20: (174, 174), 60: (163, 174), 100: (163, 174), 150: (56, 174), 300: (55, 174)}


def test_cli_prior_band_arguments():
    from svx.seg_align import align as A
    base = ["meta.tsv", "out", "--src_lang", "en", "--tgt_lang", "de", "--seg_dir", "s", "--concat_dir", "c", "--embed_dir", "e"]
    around = base + ["--mode", "around", "--prior", "time"]
    assert A.parse_args(around).prior_band is None
    assert A.parse_args(around + ["--prior_band", "80"]).prior_band == 80
    assert A.parse_args(around + ["--prior_band", "6"]).prior_band == 6
    for bad in (["--prior_band", "4"], ["--prior_band", "81"], ["--prior_band", "-8"]):
        with pytest.raises(SystemExit):
            A.parse_args(around + bad)
    with pytest.raises(SystemExit):
        A.parse_args(base + ["--mode", "band", "--prior_band", "80"])
