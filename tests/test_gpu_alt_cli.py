"""--alt_dir and --regret_dir of svx.seg_align.align on the GPU, on the trimmed shipped example (tests/golden/example_trim,
real fp16 embeddings): the alignment files do not change, and the new files are the line formatters applied to the tensors
of PreparedBatch.row_alternatives()."""
import os

import numpy as np
import pytest

from test_gpu_slack_cli import NAMES, argv, build_tree

pytestmark = pytest.mark.gpu


def test_alt_and_regret_files(tmp_path, monkeypatch):
    from svx.seg_align import align as A
    from svx.utils.file_utils import read_alignments
    from svx.vecalign import dp_utils
    root = str(tmp_path / "data")
    build_tree(root)
    plain, out, adir, rdir = (str(tmp_path / k) for k in ("plain", "out", "alt", "regret"))
    A.main(argv(root, plain, []))
    seen = []
    real = dp_utils.PreparedBatch.row_alternatives

    def spy(self, *a, **kw):
        alt = real(self, *a, **kw)
        seen.append(({k: (v.cpu().numpy().copy() if hasattr(v, "cpu") else np.asarray(v).copy()) for k, v in alt.items()},
                     np.asarray(self.offs).copy(), a, kw))
        return alt
    monkeypatch.setattr(dp_utils.PreparedBatch, "row_alternatives", spy)
    # the plain run's own files are the given paths: every row of them is a row the DP returned
    A.main(argv(root, out, ["--alt_dir", adir, "--alt_max_detour", "12", "--alt_max_slack", "0.05", "--regret_dir", rdir,
                            "--rescore_dir", plain, "--rescore_tsv", str(tmp_path / "rescore.tsv")]))
    assert len(seen) == 1   # one batch of two pairs
    alt, offs, a, kw = seen[0]
    assert a == (12, 0.05) and kw['detour'] is True
    for i, name in enumerate(NAMES):
        text = open(os.path.join(out, "en-de", name), "rb").read()
        assert text == open(os.path.join(plain, "en-de", name), "rb").read()      # the standard outputs do not change
        n = len(text.decode().splitlines())
        o = int(offs[i])
        assert alt['summary'][i, 0] == n > 0
        span = alt['span'][o:o + n]
        detours = [(alt['detour'][o + r, :span[r, 2]], alt['detour_scores'][o + r, :span[r, 2]]) if span[r, 3] == 0 else None for r in range(n)]
        want = A.format_alt_lines(alt['slack'][o:o + n], span, detours)
        got = open(os.path.join(adir, "en-de", name)).read()
        assert got == want
        assert len(got.splitlines()) == alt['summary'][i, 2] == int((span[:, 3] == 0).sum())
        for ln in got.splitlines():
            f = ln.split("\t")
            r, lo, hi = int(f[0]), int(f[2]), int(f[3])
            assert lo <= r < hi and float(f[1]) <= 0.05 + 5e-7 and 1 <= len(f) - 4 <= 12
        assert (alt['slack'][o:o + n][span[:, 3] != 2] <= 0.05).all()
        # ---- regret: the given rows are the returned ones
        g0, g1 = int(alt['given_offs'][i]), int(alt['given_offs'][i + 1])
        rows = dp_utils.given_rows_from_alignments(read_alignments(os.path.join(plain, "en-de", name)))
        assert g1 - g0 == len(rows) == n
        want = A.format_regret_lines(rows, alt['regret'][g0:g1])
        assert open(os.path.join(rdir, "en-de", name)).read() == want
        assert np.abs(alt['regret'][g0:g1]).max() < 1e-9
