"""`svx.seg_align.align --concat_max_num / --min_dur / --post_dir`: the reference's text post-filters between alignment and
margin scoring run inside the aligner job.  On two copies of the trimmed example (tests/golden/example_trim, real fp16
embeddings): the alignment files do not change, the --post_dir files are byte for byte what filter_by_cost, concat_aligns
and filter_by_dur make of the alignment files, the margin files hold exactly their lines of at most 5 x 5 segments, and the
scores match a float64 reference built from the files alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_align_margin_cli import K, NAMES, _margin_lines, _reference_scores
from test_gpu_cli import build_tree, run_cli

pytestmark = pytest.mark.gpu
FLAGS = ["--fp16_embed", "--seed", "5", "--max_cost", "0.7", "--concat_max_num", "3", "--apply_dur_cond_to_both_sides", "--min_dur", "1.0"]
WIDTH = 5   # -a 6: candidates span up to 5 segments


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("concat_cli")
    root = str(tmp / "data")
    build_tree(root, copies=2)
    plain, out, margin, post = str(tmp / "plain"), str(tmp / "out"), str(tmp / "margin"), str(tmp / "post")
    run_cli(root, plain, ["--fp16_embed", "--seed", "5"])
    run_cli(root, out, FLAGS + ["--margin_dir", margin, "--post_dir", post])
    return dict(tmp=tmp, root=root, plain=plain, out=out, margin=margin, post=post)


def _three_tools(runs):
    """filter_by_cost, concat_aligns and filter_by_dur, by their command lines, on the alignment files -> directory."""
    from svx.postprocess import concat_aligns, filter_by_cost, filter_by_dur
    tmp, root = runs["tmp"], runs["root"]
    meta, lang = os.path.join(root, "metadata.tsv"), ["--src_lang", "en", "--tgt_lang", "de"]
    cost, cat, dur = str(tmp / "tool_cost"), str(tmp / "tool_cat"), str(tmp / "tool_dur")
    if not os.path.isdir(dur):
        filter_by_cost.main([meta, cost, "--align_dir", runs["out"], "--max_cost", "0.7"] + lang)
        concat_aligns.main([meta, cat, "--max_num_align", "3", "--align_dir", cost, "--seg_dir", os.path.join(root, "seg"),
                            "--apply_dur_cond_to_both_sides"] + lang)
        filter_by_dur.main([meta, dur, "--align_dir", cat, "--seg_dir", os.path.join(root, "seg"), "--min_dur", "1.0"] + lang)
    return dur


def test_alignment_files_do_not_change(runs):
    for n in NAMES:
        assert open(os.path.join(runs["out"], "en-de", n), "rb").read() == open(os.path.join(runs["plain"], "en-de", n), "rb").read()
    for key in ("out", "margin", "post"):
        assert sorted(os.listdir(os.path.join(runs[key], "en-de"))) == NAMES   # (no temporary files left either)


def test_post_files_are_what_the_three_tools_write(runs):
    tools = _three_tools(runs)
    for n in NAMES:
        assert open(os.path.join(runs["post"], "en-de", n), "rb").read() == open(os.path.join(tools, "en-de", n), "rb").read()


def test_margin_files_hold_the_post_lines_that_fit_a_candidate(runs):
    from svx.utils.file_utils import read_alignments
    fitting = wide = 0
    for n in NAMES:
        post = read_alignments(os.path.join(runs["post"], "en-de", n))
        want = [(s, t) for s, t in post if len(s) <= WIDTH and len(t) <= WIDTH]
        got = [(s, t) for s, t, _ in _margin_lines(os.path.join(runs["margin"], "en-de", n))]
        assert got == want
        fitting += len(want)
        wide += len(post) - len(want)
        assert any(len(s) > 1 and s[0] != s[-1] for s, _ in got)     # joined alignments are among them
    print("post-filter chain on the trimmed example: %d fitting and %d wide lines" % (fitting, wide))
    assert fitting >= 2 * K, "only %d fitting rows: the search would be degenerate" % fitting
    assert wide >= 1


def test_scores_match_a_float64_reference(runs):
    """Span -> first matching cat_segs line -> .f16 row, float64 margins; 1e-5 is the bound test_gpu_align_margin_cli uses
    for the same arithmetic."""
    got = np.array([c for n in NAMES for _, _, c in _margin_lines(os.path.join(runs["margin"], "en-de", n))], np.float64)
    want = _reference_scores(runs)
    err = float(np.abs(got - want).max())
    print("margin of joined alignments from candidate rows: %d rows, max |score - float64| = %.3e" % (len(got), err))
    assert err < 1e-5, err


def test_post_dir_alone_needs_no_margin(runs):
    """--post_dir without --margin_dir: the same files, host work only."""
    out, post = str(runs["tmp"] / "out_post"), str(runs["tmp"] / "post_only")
    run_cli(runs["root"], out, FLAGS + ["--post_dir", post])
    for n in NAMES:
        assert open(os.path.join(post, "en-de", n), "rb").read() == open(os.path.join(runs["post"], "en-de", n), "rb").read()


def test_two_ranks_score_against_the_union(runs):
    """torch.distributed.run with two processes, one per GPU: each aligns one pair and scores its joined rows against both
    ranks'.  Same neighbours, different summation order: within 2e-7 of the single-rank run."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    out, margin, post = str(runs["tmp"] / "out_2"), str(runs["tmp"] / "margin_2"), str(runs["tmp"] / "post_2")
    root = runs["root"]
    env = dict(os.environ, PYTHONPATH=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech-vecalign_amd"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29693", "-m", "svx.seg_align.align", os.path.join(root, "metadata.tsv"), out,
           "--src_lang", "en", "--tgt_lang", "de", "--seg_dir", os.path.join(root, "seg"), "--concat_dir", os.path.join(root, "cat"),
           "--embed_dir", os.path.join(root, "emb"), "--ign_indices_dir", os.path.join(root, "ign")] + FLAGS + \
          ["--margin_dir", margin, "--post_dir", post]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    for n in NAMES:
        assert open(os.path.join(post, "en-de", n), "rb").read() == open(os.path.join(runs["post"], "en-de", n), "rb").read()
        one = _margin_lines(os.path.join(runs["margin"], "en-de", n))
        two = _margin_lines(os.path.join(margin, "en-de", n))
        assert [(s, t) for s, t, _ in one] == [(s, t) for s, t, _ in two]
        assert max(abs(a[2] - b[2]) for a, b in zip(one, two)) <= 2e-7
