"""--slack_dir of svx.seg_align.align on the GPU, on the trimmed shipped example (tests/golden/example_trim, real fp16
embeddings): the alignment files do not change, every slack file repeats its alignment file with a fourth field, and that
field is PreparedBatch.row_slack() to the printed digits."""
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TRIM = os.path.join(os.path.dirname(__file__), "golden", "example_trim")
NAMES = ["doc%d_en-doc%d_de.txt" % (c, c) for c in range(2)]


def build_tree(root, copies=2):
    meta = []
    for c in range(copies):
        stem = "doc%d" % c
        for lang in ("en", "de"):
            for sub in ("seg", "cat", "emb"):
                os.makedirs(os.path.join(root, sub, lang), exist_ok=True)
            shutil.copy(os.path.join(TRIM, f"segments_{lang}.txt"), os.path.join(root, "seg", lang, f"{stem}_{lang}.txt"))
            shutil.copy(os.path.join(TRIM, f"cat_segs_{lang}.txt"), os.path.join(root, "cat", lang, f"{stem}_{lang}.txt"))
            shutil.copy(os.path.join(TRIM, f"embeds_{lang}.f16"), os.path.join(root, "emb", lang, f"{stem}_{lang}.embed"))
        os.makedirs(os.path.join(root, "ign", "en-de"), exist_ok=True)
        for side in ("src", "tgt"):
            shutil.copy(os.path.join(TRIM, f"ignore_{side}.txt"), os.path.join(root, "ign", "en-de", f"{stem}_en-{stem}_de.{side}.txt"))
        meta.append(f"/audio/{stem}_en.ogg\t/audio/{stem}_de.ogg")
    with open(os.path.join(root, "metadata.tsv"), "w") as f:
        f.write("\n".join(meta) + "\n")


def argv(root, out, extra):
    return [os.path.join(root, "metadata.tsv"), out, "--src_lang", "en", "--tgt_lang", "de", "--seg_dir", os.path.join(root, "seg"),
            "--concat_dir", os.path.join(root, "cat"), "--embed_dir", os.path.join(root, "emb"),
            "--ign_indices_dir", os.path.join(root, "ign"), "--fp16_embed", "--seed", "11"] + extra


@pytest.mark.parametrize("mode", [[], ["--mode", "band", "--band", "32"]], ids=["ref", "band32"])
def test_slack_files(tmp_path, monkeypatch, mode):
    from svx.seg_align import align as A
    from svx.utils.file_utils import read_alignments_with_score, read_alignments_with_slack
    from svx.vecalign import dp_utils
    root = str(tmp_path / "data")
    build_tree(root)
    plain, out, sdir = str(tmp_path / "plain"), str(tmp_path / "out"), str(tmp_path / "slack")
    A.main(argv(root, plain, mode))
    seen = []
    real = dp_utils.PreparedBatch.row_slack

    def spy(self):
        sl, summ = real(self)
        seen.append((sl.cpu().numpy().copy(), np.asarray(self.offs).copy(), summ.cpu().numpy().copy()))
        return sl, summ
    monkeypatch.setattr(dp_utils.PreparedBatch, "row_slack", spy)
    A.main(argv(root, out, mode + ["--slack_dir", sdir]))
    assert len(seen) == 1   # one batch of two pairs
    slack, offs, summ = seen[0]
    for i, name in enumerate(NAMES):
        text = open(os.path.join(out, "en-de", name), "rb").read()
        assert text == open(os.path.join(plain, "en-de", name), "rb").read()      # the standard outputs do not change
        lines = text.decode().splitlines()
        slines = open(os.path.join(sdir, "en-de", name)).read().splitlines()
        assert len(slines) == len(lines) == summ[i, 0] > 0
        want = slack[int(offs[i]):int(offs[i]) + len(lines)]
        for ln, sln, v in zip(lines, slines, want):
            head, _, last = sln.rpartition(":")
            assert head == ln and last == "%.6f" % v
        rows = read_alignments_with_slack(os.path.join(sdir, "en-de", name))
        assert [r[:3] for r in rows] == read_alignments_with_score(os.path.join(out, "en-de", name))
        assert all(r[3] >= -1e-6 for r in rows)


def test_inf_is_written_as_inf():
    from svx.seg_align.align import format_slack_lines
    rows = np.asarray([[0, 1, 0, 1], [1, 0, 1, 1]], np.int32)
    text = format_slack_lines(rows, np.asarray([0.349737, 0.0]), np.asarray([0.012345, np.inf]))
    assert text == "[0]:[0]:0.349737:0.012345\n[]:[1]:0.000000:inf\n"


@pytest.mark.parametrize("extra,text", [(["--widen"], "cannot be combined with --widen"),
                                        (["--skip_existing"], "cannot be combined with --skip_existing"),
                                        (["--mode", "band", "--band", "80"], "runs the tile sweep, which keeps no cost array")])
def test_refused_combinations(tmp_path, capsys, extra, text):
    from svx.seg_align import align as A
    with pytest.raises(SystemExit) as e:
        A.parse_args(argv(str(tmp_path), str(tmp_path / "out"), ["--slack_dir", str(tmp_path / "s")] + extra))
    assert e.value.code == 2
    assert text in " ".join(capsys.readouterr().err.split())


def test_dense_mode_is_refused_by_the_library(tmp_path):
    """--mode dense sizes its band by the documents, so the parser cannot know: the library's error comes through."""
    from svx import _lib
    from svx.seg_align import align as A
    root = str(tmp_path / "data")
    build_tree(root, copies=1)
    with pytest.raises(_lib.SvxError, match="tile sweep, which keeps no cost array"):
        A.main(argv(root, str(tmp_path / "out"), ["--mode", "dense", "--slack_dir", str(tmp_path / "s")]))
