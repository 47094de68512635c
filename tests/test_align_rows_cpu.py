"""What the GPU tests of svx_alignment_rows rest on, without a GPU: the text threshold filters.cost_limit, the keep rule
on the reference's shipped example, and the conditions the synthetic batches of align_rows_ref must meet."""
import math
import os

import numpy as np
import pytest

import align_rows_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("max_cost", [0.7, 0.5, 0.0, 1e-6, 0.007812, 123.456789])
def test_cost_limit_is_the_text_threshold(max_cost):
    """200 doubles on each side of the limit: the double comparison agrees with the comparison of the '%.6f' text."""
    from svx.postprocess.filters import cost_limit
    limit = cost_limit(max_cost)
    assert limit >= 0 and float("%.6f" % limit) <= max_cost
    for direction in (-math.inf, math.inf):
        v = limit
        for _ in range(200):
            v = max(0.0, math.nextafter(v, direction))
            assert (v <= limit) == (float("%.6f" % v) <= max_cost), (v, limit)


def test_cost_limit_edges():
    from svx.postprocess.filters import cost_limit
    with pytest.raises(ValueError):
        cost_limit(-1.0)
    assert cost_limit(0.007812) == 0.0078125          # the exactly representable tie prints as 0.007812
    assert cost_limit(math.inf) == math.inf
    assert R.MAX_SCORE == cost_limit(0.7)


def test_shipped_example_keeps_the_lines_of_filter_by_cost():
    """The keep rule with max_score = cost_limit(0.7) on the shipped alignment file = the reference's align_0.7.txt."""
    from svx.postprocess.filters import cost_limit
    from svx.utils.file_utils import read_alignments_with_score
    rows = read_alignments_with_score(os.path.join(GOLD, "example_full", "shipped_alignment.txt"))
    assert len(rows) == 156
    n = 1 + max(s[-1] for s, _, _ in rows if s)
    m = 1 + max(t[-1] for _, t, _ in rows if t)
    k = max(max(len(s), len(t)) for s, t, _ in rows)
    align = np.array([(s[0] if s else 0, len(s), t[0] if t else 0, len(t)) for s, t, _ in rows], np.int32)
    pair = dict(v0=np.zeros((k, n, 8), np.float32), v1=np.zeros((k, m, 8), np.float32), align=align,
                scores=np.array([c for _, _, c in rows], np.float64), info=np.array([len(rows), 0], np.int32))
    kept = R.kept_rows(pair, cost_limit(0.7))
    got = ["%s:%s:%s\n" % rows[r] for r in kept]
    want = open(os.path.join(GOLD, "example_files", "align_0.7.txt")).readlines()
    assert len(want) == 145 and got == want


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_generated_batches_cannot_be_passed_by_keeping_all_or_nothing(name):
    batch = R.build(name)
    nondel, kept, at, above = R.stats(batch)
    assert nondel > 0 and 0.2 <= kept / nondel <= 0.8, (kept, nondel)
    assert at >= 1 and above >= 1
    ref = R.reference(batch, batch["max_score"])
    assert ref["count"] == kept == len(ref["src"])
    # a pair that keeps nothing stands at the start, in the middle or at the end wherever the spec says so
    for i, kind in enumerate(batch["spec"]):
        if not isinstance(kind, tuple):
            assert not (ref["src"][:, 0] == i).any()


def test_reference_restates_the_contract():
    batch = R.build("edges-d32-f16")
    T = batch["max_score"]
    ref = R.reference(batch, T, "fp16")
    src = ref["src"]
    assert (np.lexsort((src[:, 1], src[:, 0])) == np.arange(len(src))).all()       # (pair, row) ascending
    scores = np.array([batch["pairs"][p]["scores"][r] for p, r in src])
    assert (scores <= T).all() and (scores == T).any() and (np.signbit(scores) & (scores == 0)).any()
    big = max(range(len(batch["spec"])), key=lambda i: batch["spec"][i][1] if isinstance(batch["spec"][i], tuple) else -1)
    assert ((src[:, 0] == big) & (src[:, 1] == 0)).any() and ((src[:, 0] == big) & (src[:, 1] == 1)).any()   # the edge rows
    # unit rows: unit norm (or zero) in float64, to fp16 rounding
    xu = ref["x_unit"].view(np.float16).astype(np.float64)
    norms = np.sqrt((xu * xu).sum(axis=1))
    assert np.all((np.abs(norms - 1) < 1e-3) | (norms == 0))
    inf = R.reference(batch, np.inf)
    assert inf["count"] > ref["count"] and inf["x_unit"] is None
