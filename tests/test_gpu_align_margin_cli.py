"""`svx.seg_align.align --margin_dir`: the aligner job margin-scores its own alignments from the candidate rows it holds.
On two copies of the trimmed example (tests/golden/example_trim, real fp16 embeddings): the alignment files do not change,
the margin files hold exactly the lines filter_by_cost keeps, and the scores match a float64 reference built from the
files alone (alignment file -> segment span -> first matching candidate line -> row of the .f16 file)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_cli import TRIM, build_tree, run_cli

pytestmark = pytest.mark.gpu
K = 16
NAMES = ["doc%d_en-doc%d_de.txt" % (c, c) for c in range(2)]
FLAGS = ["--fp16_embed", "--seed", "5", "--max_cost", "0.7"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("margin_cli")
    root = str(tmp / "data")
    build_tree(root, copies=2)
    plain, out, margin = str(tmp / "plain"), str(tmp / "out"), str(tmp / "margin")
    run_cli(root, plain, ["--fp16_embed", "--seed", "5"])
    run_cli(root, out, FLAGS + ["--margin_dir", margin])
    return dict(tmp=tmp, root=root, plain=plain, out=out, margin=margin)


def _margin_lines(path):
    from svx.utils.file_utils import read_alignments_with_score
    return read_alignments_with_score(path)


def test_alignment_files_do_not_change(runs):
    for n in NAMES:
        assert open(os.path.join(runs["out"], "en-de", n), "rb").read() == open(os.path.join(runs["plain"], "en-de", n), "rb").read()
    assert sorted(os.listdir(os.path.join(runs["out"], "en-de"))) == NAMES   # (no temporary files left either)
    assert sorted(os.listdir(os.path.join(runs["margin"], "en-de"))) == NAMES


def test_margin_files_hold_the_lines_filter_by_cost_keeps(runs):
    from svx.postprocess.filters import keep_by_cost
    total = 0
    for n in NAMES:
        kept_path = str(runs["tmp"] / ("kept_" + n))
        keep_by_cost(os.path.join(runs["out"], "en-de", n), kept_path, max_cost=0.7)
        want = [(s, t) for s, t, _ in _margin_lines(kept_path)]
        got = [(s, t) for s, t, _ in _margin_lines(os.path.join(runs["margin"], "en-de", n))]
        assert got == want
        total += len(got)
    assert total >= 2 * K, "only %d kept rows: the search would be degenerate" % total


def _file_rows(lang):
    """-> (segments [(start, end)], candidate line -> first row, embedding rows float32) of the trimmed example."""
    segs = [tuple(l.split()) for l in open(os.path.join(TRIM, "segments_%s.txt" % lang)).read().splitlines()]
    first = {}
    for i, line in enumerate(open(os.path.join(TRIM, "cat_segs_%s.txt" % lang)).read().splitlines()):
        first.setdefault(line.strip(), i)
    emb = np.fromfile(os.path.join(TRIM, "embeds_%s.f16" % lang), dtype=np.float16).reshape(-1, 1024)
    return segs, first, emb


def _reference_scores(runs):
    """float64 margin scores of every line of the margin files, in file order, from the files alone."""
    from margin_ref import margin_f64, topk_desc, unit_f32
    from oracle import round_storage
    sides = {"en": _file_rows("en"), "de": _file_rows("de")}

    def row(lang, ids):
        segs, first, emb = sides[lang]
        return emb[first["%s %s" % (segs[ids[0]][0], segs[ids[-1]][1])]].astype(np.float32)
    x, y = [], []
    for n in NAMES:
        for s, t, _ in _margin_lines(os.path.join(runs["margin"], "en-de", n)):
            x.append(row("en", s))
            y.append(row("de", t))
    x, y = np.stack(x), np.stack(y)
    qx, qy = (round_storage(unit_f32(v)[0], "fp16").astype(np.float64) for v in (x, y))   # database rows = rounded queries
    mxy = topk_desc(qx @ qy.T, K).mean(axis=1)
    myx = topk_desc(qy @ qx.T, K).mean(axis=1)
    return margin_f64(x, y, mxy, myx, "ratio")[0]


def test_scores_match_a_float64_reference(runs):
    got = np.array([c for n in NAMES for _, _, c in _margin_lines(os.path.join(runs["margin"], "en-de", n))], np.float64)
    want = _reference_scores(runs)
    err = float(np.abs(got - want).max())
    print("margin from candidate rows: %d rows, max |score - float64| = %.3e" % (len(got), err))
    assert err < 1e-5, err


def test_one_pair_per_batch_gives_the_same_files(runs):
    """The rows of every batch wait on the device for the last one: two batches of one pair score like one batch of two
    (same database rows in the same order; 2e-7 is the bar between two summation orders of the same neighbours)."""
    out, margin = str(runs["tmp"] / "out_b1"), str(runs["tmp"] / "margin_b1")
    run_cli(runs["root"], out, FLAGS + ["--margin_dir", margin, "--batch_size", "1"])
    for n in NAMES:
        one = _margin_lines(os.path.join(runs["margin"], "en-de", n))
        two = _margin_lines(os.path.join(margin, "en-de", n))
        assert [(s, t) for s, t, _ in one] == [(s, t) for s, t, _ in two]
        assert max(abs(a[2] - b[2]) for a, b in zip(one, two)) <= 2e-7


def test_margin_dir_with_skip_existing_is_rejected(tmp_path, capsys):
    from svx.seg_align import align as A
    with pytest.raises(SystemExit):
        A.parse_args(["meta.tsv", str(tmp_path), "--src_lang", "en", "--tgt_lang", "de", "--seg_dir", "s", "--concat_dir", "c",
                      "--embed_dir", "e", "--margin_dir", str(tmp_path / "m"), "--skip_existing"])
    assert "--skip_existing" in capsys.readouterr().err


@pytest.mark.parametrize("exchange", ["allgather", "ring"])
def test_two_ranks_score_against_the_union(runs, exchange):
    """torch.distributed.run with two processes, one per GPU: each aligns one pair and scores its rows against both ranks'.
    Same neighbours, different summation order: within 2e-7 of the single-rank run."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    out, margin = str(runs["tmp"] / ("out_" + exchange)), str(runs["tmp"] / ("margin_" + exchange))
    root = runs["root"]
    env = dict(os.environ, PYTHONPATH=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech-vecalign_amd"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29691" if exchange == "ring" else "29692", "-m", "svx.seg_align.align", os.path.join(root, "metadata.tsv"), out,
           "--src_lang", "en", "--tgt_lang", "de", "--seg_dir", os.path.join(root, "seg"), "--concat_dir", os.path.join(root, "cat"),
           "--embed_dir", os.path.join(root, "emb"), "--ign_indices_dir", os.path.join(root, "ign")] + FLAGS + \
          ["--margin_dir", margin, "--margin_exchange", exchange]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    for n in NAMES:
        one = _margin_lines(os.path.join(runs["margin"], "en-de", n))
        two = _margin_lines(os.path.join(margin, "en-de", n))
        assert [(s, t) for s, t, _ in one] == [(s, t) for s, t, _ in two]
        assert max(abs(a[2] - b[2]) for a, b in zip(one, two)) <= 2e-7
