"""--rescore_dir / --rescore_tsv of svx.seg_align.align and the gold line of svx.vecalign.vecalign.align on the GPU: a
given alignment file priced with the run's own costs (svx_score_alignments), without a change to the alignment files."""
import logging
import os

import numpy as np
import pytest

import given_ref
from around_ref import block_deletion_pair

pytestmark = pytest.mark.gpu
FULL = os.path.join(os.path.dirname(__file__), "golden", "example_full")


def write_tree(root, v0, v1):
    """The block-deletion pair as a document pair on disk: one-second segments, every candidate span of up to K segments
    with its layer row as fp16 (rows i < k of layer k are spans that do not exist)."""
    for lang, v in (("en", v0), ("de", v1)):
        K, n, d = v.shape
        for sub in ("seg", "cat", "emb"):
            os.makedirs(os.path.join(root, sub, lang), exist_ok=True)
        seg = [(32000 * i, 32000 * i + 16000) for i in range(n)]
        with open(os.path.join(root, "seg", lang, f"doc0_{lang}.txt"), "w") as f:
            f.write("".join("%d %d\n" % s for s in seg))
        lines, rows = [], []
        for i in range(n):
            for k in range(min(K, i + 1)):
                lines.append("%d %d\n" % (seg[i - k][0], seg[i][1]))
                rows.append(v[k, i])
        with open(os.path.join(root, "cat", lang, f"doc0_{lang}.txt"), "w") as f:
            f.write("".join(lines))
        np.stack(rows).astype(np.float16).tofile(os.path.join(root, "emb", lang, f"doc0_{lang}.embed"))
    with open(os.path.join(root, "metadata.tsv"), "w") as f:
        f.write("/audio/doc0_en.ogg\t/audio/doc0_de.ogg\n")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """-> (root of the data tree, argv without the output directory, the rescore directory holding the truth path)."""
    tmp = tmp_path_factory.mktemp("given_cli")
    v0, v1, src = block_deletion_pair(d=1024, seed=0)
    root = str(tmp / "data")
    write_tree(root, v0, v1)
    given = tmp / "given" / "en-de"
    os.makedirs(given)
    with open(given / "doc0_en-doc0_de.txt", "w") as f:      # without scores, and only the 1-1 pairs: the gaps are deletions
        f.write("".join("%s:%s\n" % (x, y) for x, y in given_ref.truth_path(src, 300) if x and y))
    base = [os.path.join(root, "metadata.tsv"), None, "--src_lang", "en", "--tgt_lang", "de", "--seg_dir", os.path.join(root, "seg"),
            "--concat_dir", os.path.join(root, "cat"), "--embed_dir", os.path.join(root, "emb"), "--fp16_embed", "--seed", "3",
            "-a", "5", "--max_size_full_dp", "100"]
    return tmp, base, str(tmp / "given")


def run(tmp, base, name, extra):
    from svx.seg_align import align as A
    argv = list(base)
    argv[1] = str(tmp / name)
    A.main(argv + extra)
    return open(os.path.join(argv[1], "en-de", "doc0_en-doc0_de.txt"), "rb").read()


def fields(path):
    lines = open(path).read().splitlines()
    assert len(lines) == 1
    f = lines[0].split("\t")
    assert len(f) == 14 and f[:2] == ["doc0_en.txt", "doc0_de.txt"]
    return f[2], [float(x) for x in f[3:6]], [int(x) for x in f[6:]], f[3:6]


def test_band_14_is_a_search_error_and_the_reference_mode_a_model_error(tree):
    tmp, base, given = tree
    plain_band = run(tmp, base, "band", ["--mode", "band", "--band", "14"])
    band = run(tmp, base, "band_given", ["--mode", "band", "--band", "14", "--rescore_dir", given, "--rescore_tsv", str(tmp / "band.tsv")])
    assert band == plain_band                               # the alignment files do not change
    verdict, (found, got, pen), report, text = fields(tmp / "band.tsv")
    assert verdict == "search" and report == [300, 180, 120, 0, 0, 0, 206, 1]
    assert got < found - 20 and pen > 0 and all(len(t.split(".")[1]) == 6 for t in text)
    plain_ref = run(tmp, base, "ref", [])
    ref = run(tmp, base, "ref_given", ["--rescore_dir", given, "--rescore_tsv", str(tmp / "ref.tsv")])
    assert ref == plain_ref and ref != band
    verdict2, (found2, got2, pen2), report2, _ = fields(tmp / "ref.tsv")
    assert verdict2 == "model" and report2[:6] == [300, 180, 120, 0, 0, 0] and report2[6] == 0 and report2[7] == 1
    assert found2 < got2 and found2 < found and pen2 > 0     # (the two modes draw their normaliser and penalty samples differently)


def test_a_file_that_is_no_path_gives_an_invalid_line_and_a_missing_one_none(tree, caplog):
    from svx.seg_align import align as A
    tmp, base, _ = tree
    bad = tmp / "bad" / "en-de"
    os.makedirs(bad, exist_ok=True)
    with open(bad / "doc0_en-doc0_de.txt", "w") as f:
        f.write("[0]:[0]:0.1\n[2, 1]:[1]:0.2\n")
    with caplog.at_level(logging.WARNING, logger=A.logger.name):
        run(tmp, base, "bad_out", ["--mode", "band", "--band", "14", "--rescore_dir", str(tmp / "bad"), "--rescore_tsv", str(tmp / "bad.tsv")])
    assert open(tmp / "bad.tsv").read() == "doc0_en.txt\tdoc0_de.txt\tinvalid" + "\t" * 11 + "\n"
    assert any("no monotone alignment" in r.getMessage() for r in caplog.records)
    os.makedirs(tmp / "none" / "en-de", exist_ok=True)
    run(tmp, base, "none_out", ["--mode", "band", "--band", "14", "--rescore_dir", str(tmp / "none"), "--rescore_tsv", str(tmp / "none.tsv")])
    assert open(tmp / "none.tsv").read() == ""


def test_rejected_flag_combinations(tree):
    from svx.seg_align import align as A
    tmp, base, given = tree
    argv = [a if a is not None else str(tmp / "never") for a in base]
    for extra in (["--rescore_dir", given], ["--rescore_tsv", "x.tsv"],
                  ["--rescore_dir", given, "--rescore_tsv", "x.tsv", "--widen"],
                  ["--rescore_dir", given, "--rescore_tsv", "x.tsv", "--skip_existing"]):
        with pytest.raises(SystemExit):
            A.parse_args(argv + extra)
    assert A.parse_args(argv + ["--rescore_dir", given, "--rescore_tsv", "x.tsv"]).rescore_tsv == "x.tsv"


def test_shipped_example_logs_the_gold_path_at_the_aligners_prices():
    from svx.vecalign import vecalign as V
    records = []

    class Keep(logging.Handler):
        def emit(self, record):
            records.append(record.getMessage())
    handler = Keep(level=logging.INFO)
    old = V.logger.level
    V.logger.addHandler(handler)
    V.logger.setLevel(logging.INFO)
    try:
        args = V.parse_args(["-s", os.path.join(FULL, "segments_en.txt"), "-t", os.path.join(FULL, "segments_de.txt"),
                             "--src_embed", os.path.join(FULL, "cat_segs_en.txt"), os.path.join(FULL, "embeds_en.f16"), "--src_fp16",
                             "--tgt_embed", os.path.join(FULL, "cat_segs_de.txt"), os.path.join(FULL, "embeds_de.f16"), "--tgt_fp16",
                             "-a", "6", "--overlap_segments", "--src_ignore_indices", os.path.join(FULL, "ignore_src.txt"),
                             "--tgt_ignore_indices", os.path.join(FULL, "ignore_tgt.txt"), "-g", os.path.join(FULL, "gold.txt")])
        np.random.seed(0)
        stack = V.align(**vars(args))
    finally:
        V.logger.removeHandler(handler)
        V.logger.setLevel(old)
    g = stack[0]['given']
    assert g['report'] == (147, 133, 11, 3, 0, 2, 0, 1) and g['verdict'] == "unpriced"
    assert round(g['found_total'], 2) == 103.63 and round(g['given_total'], 2) == 116.25
    line = [m for m in records if "gold path at the aligner's prices" in m]
    assert len(line) == 1 and "(147, 133, 11, 3, 0, 2, 0, 1)" in line[0] and "verdict unpriced" in line[0]
    assert records.index(line[0]) == len(records) - 1            # behind the P / R / F lines
