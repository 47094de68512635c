"""The post-filter chain without a GPU: concat_rows_ref (the restatement svx_concat_rows is tested against) equals the literal
text tools keep_by_cost -> concat_consecutive -> keep_by_duration run through files, and filters.post_chain; its synthetic
batches hold every situation the GPU test relies on; the committed example reproduces the reference's 347 lines; the new
flags of seg_align.align parse."""
import os

import numpy as np
import pytest

import concat_rows_ref as C

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def _lines(outs):
    return ["%s:%s" % (list(range(o[3], o[3] + o[4])), list(range(o[5], o[5] + o[6]))) for o, _ in outs]


def _through_files(tmp, rows, f0, f1, prm):
    """filter_by_cost --max_cost 0.7, concat_aligns, filter_by_dur on the alignment file written from `rows`."""
    from svx.postprocess import filters
    from svx.utils.file_utils import read_alignments, read_lines, write_alignment
    paths = {k: os.path.join(tmp, k + ".txt") for k in ("align", "cost", "cat", "dur", "seg0", "seg1")}
    for key in paths.values():
        if os.path.exists(key):
            os.remove(key)
    with open(paths["align"], "w") as fp:
        fp.writelines("%s:%s:%.6f\n" % r for r in rows)
    for key, fr in (("seg0", f0), ("seg1", f1)):
        with open(paths[key], "w") as fp:
            fp.writelines("%d %d\n" % tuple(v) for v in fr)
    if not rows:
        return []
    filters.keep_by_cost(paths["align"], paths["cost"], max_cost=0.7)
    if not os.path.exists(paths["cost"]):
        return []
    write_alignment(filters.concat_consecutive(read_alignments(paths["cost"]), f0, f1, prm["max_num_align"], prm["max_sil"], prm["max_dur"],
                                               prm["sample_rate"], bool(prm["both_sides"])), paths["cat"])
    filters.keep_by_duration(paths["cat"], paths["seg0"], paths["seg1"], prm["min_frames"], paths["dur"])
    return read_lines(paths["dur"]) if os.path.exists(paths["dur"]) else []


@pytest.mark.parametrize("prm", [C.PARAMS, C.params(both_sides=0, max_num_align=8), C.params(max_num_align=1), C.params(max_num_align=2, min_frames=0)],
                         ids=["cat3", "cat8-src-only", "no-joining", "cat2-no-min"])
def test_restatement_equals_the_text_tools_and_post_chain(tmp_path, prm):
    from svx.postprocess import filters
    assert C.MAX_SCORE == filters.cost_limit(0.7)
    batch = C.build("edges-d32-f16")
    checked = 0
    for pair in batch["pairs"]:
        if pair["info"][1] != 0:
            continue                                   # (a failed pair has no alignment file)
        rows, f0, f1 = C.as_lists(pair)
        want = _lines(C.chain_outputs(pair, prm))
        assert _through_files(str(tmp_path), rows, f0, f1, prm) == want
        got = filters.post_chain(rows, f0, f1, 0.7, prm["max_num_align"], prm["max_sil"], prm["max_dur"], bool(prm["both_sides"]), prm["min_frames"])
        assert ["%s:%s" % st for st in got] == want
        checked += len(want)
    assert checked > 1000


def test_every_planted_situation_is_there():
    batch = C.build("edges-d32-f16")
    for both in (0, 1):
        got = C.classes(batch, C.params(both_sides=both))
        assert all(v > 0 for v in got.values()), got
    assert C.classes(batch, C.params(both_sides=0))["joined"] == C.classes(batch, C.PARAMS)["joined"] + 1   # group H of the equality pair
    kinds = [k if isinstance(k, str) else k[0] for k in batch["spec"]]
    none = [i for i, k in enumerate(kinds) if k in ("all_del", "zero_info", "failed")]
    assert none[0] == 0 and none[-1] == len(kinds) - 1 and 0 < none[1] < len(kinds) - 1
    assert sorted(kinds[i] for i in none) == ["all_del", "failed", "zero_info"]
    failed = batch["pairs"][kinds.index("failed")]
    assert failed["info"][1] != 0 and (np.abs(failed["align"].astype(np.int64)) >= 1 << 30).any()   # out-of-range garbage
    assert {int(p["info"][0]) for p, k in zip(batch["pairs"], batch["spec"]) if isinstance(k, tuple) and k[0] == "rows"} == {0, 1, 255, 256, 257, 513, 1100}
    ref = C.reference(batch, C.PARAMS)
    assert ref["count"] > 256 * 3 and ref["wide"] > 0
    assert C.reference(C.build("no-rows"), C.PARAMS)["count"] == 0
    # every case the GPU tests run forms joined rows (or none at all, "no-rows")
    tiny = C.reference(C.build("tiny-pairs"), C.PARAMS)
    assert tiny["count"] > 1024 and (tiny["meta"][:, 3] > 1).any()


def test_the_committed_example_gives_the_references_347_lines():
    """align_0.7_clean.txt -> concat_aligns --max_num_align 3 --max_dur 20 --apply_dur_cond_to_both_sides -> filter_by_dur
    --min_dur 1.0 is the committed align_0.7_clean_cat3_min1s.txt; 307 of its lines span at most 5 x 5 segments (-a 6)."""
    from svx.postprocess import filters
    from svx.utils.file_utils import read_alignments_with_score, read_lines, read_segments
    rows = read_alignments_with_score(os.path.join(GOLD, "example_files", "align_0.7_clean.txt"))
    f0 = read_segments(os.path.join(GOLD, "example_full", "segments_en.txt"))
    f1 = read_segments(os.path.join(GOLD, "example_full", "segments_de.txt"))
    got = filters.post_chain(rows, f0, f1, 0.7, 3, 1.0, 20.0, True, 16000)
    want = read_lines(os.path.join(GOLD, "example_files", "align_0.7_clean_cat3_min1s.txt"))
    assert len(want) == 347 and ["%s:%s" % st for st in got] == want
    assert sum(1 for s, t in got if len(s) <= 5 and len(t) <= 5) == 307
    # the restatement on the same rows
    n, m = len(f0), len(f1)
    align = np.zeros((n + m + 2, 4), np.int32)
    align[:len(rows)] = [(s[0], len(s), t[0], len(t)) for s, t, _ in rows]
    scores = np.zeros(n + m + 2)
    scores[:len(rows)] = [c for _, _, c in rows]
    pair = dict(v0=np.zeros((5, n, 1)), v1=np.zeros((5, m, 1)), align=align, scores=scores, info=np.array([len(rows), 0], np.int32),
                f0=np.asarray(f0, np.int32), f1=np.asarray(f1, np.int32))
    outs = C.chain_outputs(pair, C.PARAMS)
    assert _lines(outs) == want and sum(fits for _, fits in outs) == 307


def test_the_new_flags_parse():
    from svx.seg_align import align
    base = ["meta.txt", "out", "--src_lang", "en", "--tgt_lang", "de", "--seg_dir", "s", "--concat_dir", "c", "--embed_dir", "e"]
    a = align.parse_args(base)
    assert (a.concat_max_num, a.min_dur, a.post_dir, a.max_sil, a.concat_max_dur, a.apply_dur_cond_to_both_sides) == (None, None, None, 1.0, 20.0, False)
    assert not align.post_chain_wanted(a)
    a = align.parse_args(base + ["--margin_dir", "m", "--max_cost", "0.7", "--concat_max_num", "3", "--max_sil", "0.5", "--concat_max_dur", "15",
                                 "--apply_dur_cond_to_both_sides", "--min_dur", "1.0", "--post_dir", "p"])
    assert align.post_chain_wanted(a)
    assert align.post_chain_params(a) == dict(max_num_align=3, max_sil=0.5, max_dur=15.0, both_sides=True, min_frames=16000)
    assert align.post_chain_params(align.parse_args(base + ["--post_dir", "p"])) == dict(max_num_align=1, max_sil=1.0, max_dur=20.0, both_sides=False, min_frames=0)
    for bad in (["--concat_max_num", "0", "--post_dir", "p"], ["--concat_max_num", "9", "--post_dir", "p"], ["--concat_max_num", "3"],
                ["--min_dur", "-1", "--post_dir", "p"], ["--post_dir", "p", "--skip_existing"]):
        with pytest.raises(SystemExit):
            align.parse_args(base + bad)
