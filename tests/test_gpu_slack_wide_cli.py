"""--slack_wide_dir of svx.seg_align.align on the GPU, on the trimmed shipped example (tests/golden/example_trim, real fp16
embeddings) in a band of 80 cells (the tile sweep): the alignment files do not change, every slack file repeats its
alignment file with a fourth field, and that field is PreparedBatch.row_slack_wide() to the printed digits."""
import os

import numpy as np
import pytest

from test_gpu_slack_cli import NAMES, argv, build_tree

pytestmark = pytest.mark.gpu


def test_slack_wide_files(tmp_path, monkeypatch):
    from svx.seg_align import align as A
    from svx.utils.file_utils import read_alignments_with_score, read_alignments_with_slack
    from svx.vecalign import dp_utils
    root = str(tmp_path / "data")
    build_tree(root)
    mode = ["--mode", "band", "--band", "80"]
    plain, out, sdir = str(tmp_path / "plain"), str(tmp_path / "out"), str(tmp_path / "slack")
    A.main(argv(root, plain, mode))
    seen = []
    real = dp_utils.PreparedBatch.row_slack_wide

    def spy(self, *a, **kw):
        sl, summ = real(self, *a, **kw)
        seen.append((sl.cpu().numpy().copy(), np.asarray(self.offs).copy(), summ.cpu().numpy().copy()))
        return sl, summ
    monkeypatch.setattr(dp_utils.PreparedBatch, "row_slack_wide", spy)
    A.main(argv(root, out, mode + ["--slack_wide_dir", sdir]))
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
            assert head == ln and last == "%.6f" % v and sln.count(":") == 3      # four fields
        rows = read_alignments_with_slack(os.path.join(sdir, "en-de", name))
        assert [r[:3] for r in rows] == read_alignments_with_score(os.path.join(out, "en-de", name))
        assert all(r[3] >= -1e-6 for r in rows)


def test_dense_mode_picks_the_entry_per_batch(tmp_path, monkeypatch):
    """--mode dense sizes the band by the batch's documents.  A batch of short documents (20 x 18 rows: a band of 42 cells)
    runs the band kernels and keeps its cost array, the next batch (48 x 44: 98 cells) runs the tile sweep: one
    --slack_wide_dir serves both, the first through row_slack(), the second through row_slack_wide()."""
    from svx.seg_align import align as A
    from svx.vecalign import dp_utils
    root = str(tmp_path / "data")
    build_tree(root)
    for lang, keep in (("en", 20), ("de", 18)):
        seg = os.path.join(root, "seg", lang, f"doc0_{lang}.txt")
        lines = open(seg).readlines()
        assert len(lines) > 31
        open(seg, "w").writelines(lines[:keep])
    mode = ["--mode", "dense", "--batch_size", "1"]
    plain, out, sdir = str(tmp_path / "plain"), str(tmp_path / "out"), str(tmp_path / "slack")
    A.main(argv(root, plain, mode))
    seen = {}
    for entry in ("row_slack", "row_slack_wide"):
        def spy(self, *a, _real=getattr(dp_utils.PreparedBatch, entry), _entry=entry, **kw):
            sl, summ = _real(self, *a, **kw)
            seen.setdefault(_entry, []).append((int(self.vecs[0][0].shape[1]), sl.cpu().numpy().copy(), summ.cpu().numpy().copy()))
            return sl, summ
        monkeypatch.setattr(dp_utils.PreparedBatch, entry, spy)
    A.main(argv(root, out, mode + ["--slack_wide_dir", sdir]))
    assert [v[0] for v in seen["row_slack"]] == [20] and [v[0] for v in seen["row_slack_wide"]] == [48]
    for name, entry in zip(NAMES, ("row_slack", "row_slack_wide")):
        _, slack, summ = seen[entry][0]
        text = open(os.path.join(out, "en-de", name), "rb").read()
        assert text == open(os.path.join(plain, "en-de", name), "rb").read()
        lines = text.decode().splitlines()
        slines = open(os.path.join(sdir, "en-de", name)).read().splitlines()
        assert len(slines) == len(lines) == summ[0, 0] > 0
        for ln, sln, v in zip(lines, slines, slack[:len(lines)]):
            head, _, last = sln.rpartition(":")
            assert head == ln and last == "%.6f" % v
