"""The two command lines with --mode band|dense and type sets beyond the two LDS-resident tile shapes, on the trimmed
example (tests/golden/example_trim, real fp16 embeddings): svx.seg_align.align -a 8 (28 types) and
svx.vecalign.vecalign with its default -a 10 (45 types).  Each run is compared with the oracle's straight path
(make_sparse_costs + sparse_dp + sparse_traceback on search_path) on the same candidate tensors -- captured where
the command line hands them to the aligner -- and the same random stream: identical spans, scores within 1e-4."""
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TRIM = os.path.join(os.path.dirname(__file__), "golden", "example_trim")
SCORE_TOL = 1e-4


def build_tree(root):
    stem = "doc0"
    for lang in ("en", "de"):
        for sub in ("seg", "cat", "emb"):
            os.makedirs(os.path.join(root, sub, lang), exist_ok=True)
        shutil.copy(os.path.join(TRIM, f"segments_{lang}.txt"), os.path.join(root, "seg", lang, f"{stem}_{lang}.txt"))
        shutil.copy(os.path.join(TRIM, f"cat_segs_{lang}.txt"), os.path.join(root, "cat", lang, f"{stem}_{lang}.txt"))
        shutil.copy(os.path.join(TRIM, f"embeds_{lang}.f16"), os.path.join(root, "emb", lang, f"{stem}_{lang}.embed"))
    os.makedirs(os.path.join(root, "ign", "en-de"), exist_ok=True)
    for side in ("src", "tgt"):
        shutil.copy(os.path.join(TRIM, f"ignore_{side}.txt"), os.path.join(root, "ign", "en-de", f"{stem}_en-{stem}_de.{side}.txt"))
    with open(os.path.join(root, "metadata.tsv"), "w") as f:
        f.write(f"/audio/{stem}_en.ogg\t/audio/{stem}_de.ogg\n")


def host(t):
    return t.float().cpu().numpy().copy()


def straight_oracle(orc, v0, v1, types, W, rs):
    N, M = v0.shape[1], v1.shape[1]
    a, b = v0.copy(), v1.copy()
    orc.make_norm1(a)
    orc.make_norm1(b)
    n0, n1 = orc.compute_norms(a, b, 100, rs), orc.compute_norms(b, a, 100, rs)
    pen, _ = orc.make_del_penalty(a[0], b[0], n0[0], n1[0], 20000, 0.2, rs)
    path = orc.search_path([(list(range(N)), list(range(M)))], False, N, M)
    f, bo = orc.make_sparse_costs(a, b, n0, n1, path, types, W)
    return orc.sparse_traceback(*orc.sparse_dp(f, bo, types, pen, N, M), N, M)


@pytest.mark.parametrize("extra", [["--mode", "dense"], ["--mode", "band", "--band", "80"]], ids=["dense", "band80"])
def test_seg_align_cli_a8(orc, tmp_path, monkeypatch, extra):
    from svx.seg_align import align as A
    from svx.seg_align.align import pair_rng
    from svx.utils.file_utils import read_alignments_with_score
    from svx.vecalign import dp_utils
    seen = []
    real = dp_utils.PreparedBatch

    class Capture(real):
        def __init__(self, pairs, types, frac, w2, *a, **k):
            seen.append(([(host(v0), host(v1)) for v0, v1 in pairs], list(types), w2, k.get("search")))
            super().__init__(pairs, types, frac, w2, *a, **k)

    monkeypatch.setattr(dp_utils, "PreparedBatch", Capture)
    root, out = str(tmp_path / "data"), str(tmp_path / "out")
    build_tree(root)
    A.main([os.path.join(root, "metadata.tsv"), out, "--src_lang", "en", "--tgt_lang", "de", "--seg_dir", os.path.join(root, "seg"),
            "--concat_dir", os.path.join(root, "cat"), "--embed_dir", os.path.join(root, "emb"),
            "--ign_indices_dir", os.path.join(root, "ign"), "--fp16_embed", "--seed", "3", "-a", "8"] + extra)
    assert len(seen) == 1 and seen[0][3] == "straight"
    (v0, v1), = seen[0][0]
    types, w2 = seen[0][1], seen[0][2]
    assert len(types) == 28 and 2 * w2 > 64   # past the LDS-resident shapes, on the tile sweep
    al_o, sc_o = straight_oracle(orc, v0, v1, types, w2, pair_rng(3, 0))
    got = read_alignments_with_score(os.path.join(out, "en-de", "doc0_en-doc0_de.txt"))
    assert [(list(a), list(b)) for a, b, _ in got] == [(list(a), list(b)) for a, b in al_o]
    assert max(abs(g[2] - s) for g, s in zip(got, sc_o)) < SCORE_TOL + 5e-7  # (the file has 6 decimals)


def test_vecalign_cli_default_a10_dense(orc, monkeypatch):
    from svx.vecalign import dp_utils
    from svx.vecalign import vecalign as V
    seen = []
    real = dp_utils.align_band

    def capture(v0, v1, types, frac, w2, *a, **k):
        rs = np.random.RandomState()
        rs.set_state(np.random.get_state())
        seen.append((host(v0), host(v1), list(types), w2, rs))
        return real(v0, v1, types, frac, w2, *a, **k)

    monkeypatch.setattr(dp_utils, "align_band", capture)
    args = V.parse_args(["-s", os.path.join(TRIM, "segments_en.txt"), "-t", os.path.join(TRIM, "segments_de.txt"),
                         "--src_embed", os.path.join(TRIM, "cat_segs_en.txt"), os.path.join(TRIM, "embeds_en.f16"), "--src_fp16",
                         "--tgt_embed", os.path.join(TRIM, "cat_segs_de.txt"), os.path.join(TRIM, "embeds_de.f16"), "--tgt_fp16",
                         "--mode", "dense"])
    assert args.alignment_max_size == 10 and args.many_to_one is None
    np.random.seed(5)
    stack = V.align(**vars(args))
    assert len(seen) == 1
    v0, v1, types, w2, rs = seen[0]
    assert len(types) == 45 and 2 * w2 > 64
    al_o, sc_o = straight_oracle(orc, v0, v1, types, w2, rs)
    assert stack[0]['final_alignments'] == al_o
    assert np.abs(np.asarray(stack[0]['alignment_scores']) - np.asarray(sc_o)).max() < SCORE_TOL
