"""slack_wide_ref (the fused scheme of the backward tile sweep: per-diagonal cut minima with the own-edge exclusion, edges
owned by the tile of u) against slack_ref, the normative text, and against brute force over slack_ref.edges (CPU only);
and the parser rules of --slack_wide_dir.

Both sides take minima of the same singly rounded float64 sums, so every comparison is ==."""
import os

import numpy as np
import pytest

import dp_ref
import slack_ref
import slack_wide_ref
from synth import alignment_types
from test_slack_ref_cpu import CASES, case_id, make_case

T5, T6 = alignment_types(5), alignment_types(6)

# The family-Z cases of tests/test_gpu_row_slack_wide.py: sizes, types, W, levels, seed (zero embeddings: storage is irrelevant)
Z_CASES = {
    "a5_W40": ([(300, 280)], T5, 40, dp_ref.LEVELS2, 22),
    "a6_W33_bf16": ([(330, 310)], T6, 33, dp_ref.LEVELS6, 23),
    "below_one_tile": ([(20, 25)], T5, 40, dp_ref.LEVELS2, 51),
    "tile_corners": ([(64, 96)], T5, 40, dp_ref.LEVELS2, 52),
    "steep": ([(330, 120)], T5, 120, dp_ref.LEVELS2, 53),
    "dense": ([(150, 140)], T5, 200, dp_ref.LEVELS2, 54),
    "batch3_a6_W60": ([(210, 200), (330, 310), (120, 260)], T6, 60, dp_ref.LEVELS2, 55),
}


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", list(Z_CASES))
def test_fused_scheme_is_slack_ref_on_the_oracles_straight_stacks(orc, name):
    sizes, types, W, levels, seed = Z_CASES[name]
    case = (name, sizes, types, W, "f32", 32, levels, seed)
    for k, (v0, v1, n0, n1, sd) in enumerate(dp_ref.z_straight_pairs(case)):
        st = dp_ref.straight_stack(orc, v0, v1, types, W, sd, norms=(n0, n1))
        n, m = st['size0'], st['size1']
        args = (st['a_b_costs'], st['b_offset'], types, st['del_penalty'], n, m)
        rows = slack_ref.traceback(st['a_b_xp'], st['a_b_yp'], st['new_b_offset'], st['a_b_costs'].shape[2], n, m)
        bk = slack_ref.backward(*args)
        want = slack_ref.slack(*args, st['a_b_csum'], bk, rows)
        for tile in (32, 7):   # the result does not depend on who owns an edge
            got, cutmin, bk2 = slack_wide_ref.fused(*args, st['a_b_csum'], rows, tile=tile)
            assert same(got, want), (name, k, tile, np.flatnonzero(got != want)[:5])
            assert np.array_equal(bk2, bk)
        assert not np.isnan(want).any() and (want > 0.0).any()
        # ties: every case but dp_ref.Z_STRAIGHT's a6_W33_bf16, whose six normaliser levels leave no two paths with equal
        # float64 totals (226 rows, smallest slack 1.1e-13: ties of exact arithmetic that rounding breaks)
        assert (want == 0.0).any() == (name != "a6_W33_bf16"), name
        # rows that are no edges get NaN, and a row that is not the path's does not disturb the others
        bad = np.asarray([(-1, 1, 0, 1), (0, 0, 0, 0), (0, 1, 0, 9), (n, 1, m, 1), (2 ** 30, 1, 2 ** 30, 1)], np.int64)
        assert np.isnan(slack_wide_ref.fused(*args, st['a_b_csum'], bad)[0]).all()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fused_scheme_vs_brute_force_over_the_edge_list(case):
    """Lattices up to 5 x 5, every edge of E and E_b one by one (slack_ref.edges): alt[r] is the minimum over the edges that
    cross the row's cut, the row's own left out."""
    N, M, a, band, mode = case
    costs, bo, types, pen, N, M = make_case(N, M, a, band, mode, 31 * N + 7 * M + a)
    B = costs.shape[2]
    bout = slack_ref.b_offset_out(bo)
    mv = dp_ref._moves(types)
    csum, xp, yp, _ = dp_ref.sparse_dp(costs, bo, types, pen, N, M)
    end = slack_ref.end_cell(bout, B, N, M)
    if not np.isfinite(csum[end]):
        return
    rows = slack_ref.traceback(xp, yp, bout, B, N, M)
    bk = slack_ref.backward(costs, bo, types, pen, N, M)
    edges = slack_ref.edges(costs, bo, types, pen, N, M)
    for tile in (32, 2, 1):   # one tile, several, one node per tile
        got, cutmin, bk2 = slack_wide_ref.fused(costs, bo, types, pen, N, M, csum, rows, tile=tile)
        assert np.array_equal(bk2, bk)
        for r, (x0, xl, y0, yl) in enumerate(rows.tolist()):
            c, bu = x0 + y0, y0 - int(bout[x0 + y0])
            alt = min(((csum[au, b0] + w) + bk[av, b1] for au, b0, av, b1, t, w in edges
                       if au <= c < av and not (au == c and b0 == bu and mv[t] == (xl, yl))), default=np.inf)
            assert got[r] == alt - csum[end], (tile, r, rows[r])
            assert cutmin[c] == alt
        assert same(got, slack_ref.slack(costs, bo, types, pen, N, M, csum, bk, rows))


# ------------------------------------------------------------------------------------------ the parser
def argv(root, out, extra):
    return [os.path.join(root, "metadata.tsv"), out, "--src_lang", "en", "--tgt_lang", "de", "--seg_dir", os.path.join(root, "seg"),
            "--concat_dir", os.path.join(root, "cat"), "--embed_dir", os.path.join(root, "emb"),
            "--ign_indices_dir", os.path.join(root, "ign"), "--fp16_embed", "--seed", "11"] + extra


@pytest.mark.parametrize("extra", [["--mode", "band", "--band", "80"], ["--mode", "band", "--band", "66", "-a", "2"], ["--mode", "dense"],
                                   ["--mode", "around", "--prior_band", "128", "--prior", "time"], ["--mode", "band", "-a", "5"]],
                         ids=lambda e: "_".join(e).replace("--", ""))
def test_slack_wide_dir_accepted(tmp_path, extra):
    from svx.seg_align import align as A
    args = A.parse_args(argv(str(tmp_path), str(tmp_path / "out"), ["--slack_wide_dir", str(tmp_path / "s")] + extra))
    assert args.slack_wide_dir == str(tmp_path / "s") and args.slack_dir is None


@pytest.mark.parametrize("extra,text", [
    ([], "this band keeps its cost array, use --slack_dir"),                                        # --mode ref
    (["--mode", "band", "--band", "64"], "this band keeps its cost array, use --slack_dir"),
    (["--mode", "around", "--prior_band", "40", "--prior", "time"], "this band keeps its cost array, use --slack_dir"),
    (["--mode", "band", "--band", "80", "-a", "7"], "take the general tile shape"),
    (["--mode", "band", "--band", "80", "--skip_existing"], "cannot be combined with --skip_existing"),
    (["--mode", "band", "--band", "80", "--widen"], "cannot be combined with --widen"),
    (["--mode", "band", "--band", "80", "--slack_dir", "x"], "measure the same rows"),
])
def test_slack_wide_dir_refused(tmp_path, capsys, extra, text):
    from svx.seg_align import align as A
    with pytest.raises(SystemExit) as e:
        A.parse_args(argv(str(tmp_path), str(tmp_path / "out"), ["--slack_wide_dir", str(tmp_path / "s")] + extra))
    assert e.value.code == 2
    err = " ".join(capsys.readouterr().err.split())
    assert text in err and "--slack_dir" in err


def test_tile_shape_twin():
    from svx.vecalign.dp_utils import tile_shape
    assert [tile_shape(alignment_types(a)) for a in (2, 5, 6, 7, 10)] == [0, 0, 1, 2, 2]
    assert tile_shape([(1, 1), (9, 1)]) == 2 and tile_shape([(8, 8)]) == 0
