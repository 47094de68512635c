"""The properties the GPU checks of test_gpu_group_search.py rest on; no GPU.

1. The lattice group sets: coverage of the sizes, dimensions, k, orders and instantiations; group starts that are no
   multiple of the 32-row tile; queries that tie at the k-th place in every group that has queries and a (k+1)-th row.
2. search_groups_exact is search_exact of the full matrix with everything outside a group's range masked out.
3. The lattice document pairs of the mining test: both directions exact in fp32.
4. One global stable sort + greedy + partition equals the per-group passes, for all four retrievals, on random scores with
   many exact ties.
5. The example rows of tests/golden/example_full under the three cuts: ambiguous positions stay under
   search_ref.AMBIGUOUS_CAP per group, direction and storage; a block's bound is rows_search_reference's.
6. The CLI's host logic: pair list -> batches under --batch_rows, shards partition the pair list, a count mismatch is
   skipped."""
import os

import numpy as np
import pytest

import group_search_ref as gr
import margin_ref as mr
import mine_ref as mnr
import search_ref as sr

GD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 16

# the lattice document pairs of the mining test: (d, k, storage, order, seed, [(source rows, target rows)])
MINE_PAIRS = {
    "h_d96_k15": (96, 15, "fp16", "rising", 73, [(65, 120), (15, 15), (10, 40), (130, 70), (40, 14), (33, 64)]),
    "b_d544_k16": (544, 16, "bf16", "repeated", 6, [(64, 241), (16, 70), (70, 15), (129, 65)]),
}


# ---- 1
def all_sets():
    for name, (d, k, storage, qtype, order, seed, groups) in gr.LATTICE_SETS.items():
        yield name, d, k, storage, qtype, order, seed, gr.resolve_counts(groups, k)
    name, d, k, storage, qtype, order, seed, n_groups = gr.MANY
    yield name, d, k, storage, qtype, order, seed, gr.many_counts(n_groups, seed)


def test_lattice_sets_cover():
    sets = list(all_sets())
    assert {s[1] for s in sets} == {32, 96, 544, 992, 1024}
    assert {s[2] for s in sets} == {1, 15, 16, 24, 64}
    assert {s[5] for s in sets} == set(mr.ORDERS)
    assert {(s[3], s[4]) for s in sets} == {(a, b) for a in mr.STORAGES for b in mr.QTYPES}
    seen_q, seen_db = set(), set()
    for name, (d, k, *_, groups) in gr.LATTICE_SETS.items():
        seen_q |= {nq for nq, _ in groups}
        seen_db |= {N for _, N in groups}
    assert seen_q == set(gr.Q_COUNTS) and seen_db == set(gr.DB_COUNTS)
    # group starts off the 32-row tile and off the 64-query workgroup, in every set with more than one group
    for name, d, k, storage, qtype, order, seed, counts in sets:
        q_off, db_off = gr.offsets(counts)
        if len(counts) > 1:
            assert (db_off[1:-1] % 32 != 0).any() and (q_off[1:-1] % 64 != 0).any(), name
    # the many-groups case: >= 300 groups of 40 .. 70 queries, more than 256 workgroups, most last workgroups partly masked
    counts = sets[-1][-1]
    nq = np.asarray([c[0] for c in counts])
    assert len(counts) >= 300 and nq.min() >= 40 and nq.max() <= 70 and sets[-1][1] in (32, 96)
    assert int(((nq + 63) // 64).sum()) > 256 and (nq % 64 != 0).mean() > 0.9
    assert any(len(s[-1]) == 1 for s in sets)   # a single group: plain search


@pytest.mark.parametrize("name", [s[0] for s in all_sets()])
def test_lattice_sets_tie(name):
    _, d, k, storage, qtype, order, seed, counts = next(s for s in all_sets() if s[0] == name)
    q, db, q_off, db_off, sims = gr.lattice_groups(counts, d, k, seed, order)
    assert q.shape == (q_off[-1], d) and db.shape == (db_off[-1], d)
    for a in (q, db):   # every value is exact in both storage types
        assert np.array_equal(mr.round_storage(a, "fp16"), a) and np.array_equal(mr.round_storage(a, "bf16"), a)
    n_tied = 0
    for (nq, N), S in zip(counts, sims):
        assert S.shape == (nq, N)
        assert np.array_equal(S.astype(np.float32).astype(np.float64), S)
        if nq and N > k:
            assert sr.tie_shares(S, k)[0] > 0, "%s: a group of %d x %d has no tie at the k-th place" % (name, nq, N)
            n_tied += 1
    assert n_tied >= 1


def test_leak_groups_tie():
    for N in gr.LEAK_DB_ROWS:
        q, db, q_off, db_off, sims = gr.leak_groups(6, 70, N, 96, 16, 5)
        assert np.array_equal(db[0:N], db[2 * N:3 * N]) and np.array_equal(db[0:N], db[N:2 * N][::-1])
        for S in sims:
            assert sr.tie_shares(S, 16)[0] > 0 if N > 16 else S.shape == (70, N)
        full = mr.lattice_sims(q, db)
        for g in range(1, 5):
            lo, hi = int(db_off[g]), int(db_off[g + 1])
            rows = slice(int(q_off[g]), int(q_off[g + 1]))
            # the j-th row outside either end of the range is the j-th row inside it: it ties with a row of the group
            assert np.array_equal(db[lo - N:lo][::-1], db[lo:hi]) and np.array_equal(db[hi:hi + N][::-1], db[lo:hi])
            # and where the best rows meet (rising ends, falling starts) the row just outside ties with the group's best
            edge = hi if g % 2 == 0 else lo - 1
            assert np.array_equal(full[rows, edge], full[rows, hi - 1 if g % 2 == 0 else lo])
            # ... and belongs to the 16 best of the range for most queries (`rising` trends upward, row by row it need not)
            share = float((full[rows, edge] >= np.sort(full[rows, lo:hi], axis=1)[:, -min(16, N)]).mean())
            assert share > 0.5, share


# ---- 2
def test_search_groups_exact_is_masked_search():
    counts = gr.resolve_counts(gr.LATTICE_SETS["b_f32_d32_k24"][6], 24)
    q, db, q_off, db_off, sims = gr.lattice_groups(counts, 32, 24, 14, "repeated")
    full = mr.lattice_sims(q, db)
    masked = np.full(full.shape, -np.inf)
    for g in range(len(counts)):
        masked[q_off[g]:q_off[g + 1], db_off[g]:db_off[g + 1]] = sims[g]
        assert np.array_equal(full[q_off[g]:q_off[g + 1], db_off[g]:db_off[g + 1]], sims[g])
    want = sr.search_exact(masked, 24)
    got = gr.search_groups_exact(sims, 24, db_off)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(gr.search_groups_exact(gr.blocks(full, q_off, db_off), 24, db_off)[1], want[1])
    for g in range(len(counts)):   # every id lies in its group's range
        ids = got[1][q_off[g]:q_off[g + 1]]
        assert ((ids == -1) | ((ids >= db_off[g]) & (ids < db_off[g + 1]))).all()
    v, i = gr.search_groups_exact([], 5, np.zeros(1, np.int64))
    assert v.shape == i.shape == (0, 5)


# ---- 3
@pytest.mark.parametrize("case", list(MINE_PAIRS))
def test_lattice_pairs_exact(case):
    d, k, storage, order, seed, counts = MINE_PAIRS[case]
    x, y, x_off, y_off, S_xy, S_yx, yqs = gr.lattice_pairs(counts, d, k, storage, seed, order)
    m = int(np.log2(mr.pow4_floor(d))) // 2
    frac_bits = 10 if storage == "fp16" else 7
    assert any(n < k or N < k for n, N in counts) and sum(n >= k and N >= k for n, N in counts) >= 3
    for g, (n, N) in enumerate(counts):
        xg, yq = x[x_off[g]:x_off[g + 1]], yqs[g]
        for S in (S_xy[g], S_yx[g]):
            assert np.array_equal(S.astype(np.float32).astype(np.float64), S)
        # y in x: every product is a multiple of u and the absolute sum of a row's products stays below 2^24 u, so every
        # partial sum is exact in fp32 whatever its order (test_mine_ref_cpu.py's argument)
        nz = np.abs(yq[yq != 0]).astype(np.float64)
        u = 2.0 ** (np.floor(np.log2(nz.min())) - frac_bits - m)
        assert (np.abs(yq.astype(np.float64)) @ np.abs(xg.astype(np.float64)).T).max() < 2.0 ** 24 * u
        assert np.array_equal(np.rint(S_yx[g] / u) * u, S_yx[g])
    # the reference leaves out the pairs below k rows, and the others produce pairs
    out = gr.mine_local_ref(S_xy, S_yx, k, "distance", "max")
    assert out[4] == sum(n < k or N < k for n, N in counts)
    assert set(out[3].tolist()) == {g for g, (n, N) in enumerate(counts) if n >= k and N >= k}
    assert (np.diff(out[3]) >= 0).all()


# ---- 4
@pytest.mark.parametrize("retrieval", mnr.RETRIEVALS)
def test_global_select_equals_per_group(retrieval):
    rs = np.random.RandomState(9)
    for trial in range(6):
        counts = [(int(a), int(b)) for a, b in zip(rs.randint(0, 40, size=12), rs.randint(0, 40, size=12))]
        x_off, y_off = gr.offsets(counts)
        n_x, n_y = int(x_off[-1]), int(y_off[-1])
        gx = np.searchsorted(x_off, np.arange(n_x), side="right") - 1
        gy = np.searchsorted(y_off, np.arange(n_y), side="right") - 1
        # best rows inside the row's own group (-1 where the other side is empty, and for a few rows besides); scores from a
        # handful of values, so that exact ties are everywhere, across groups too
        fwd = np.array([rs.randint(y_off[g], y_off[g + 1]) if y_off[g + 1] > y_off[g] and rs.rand() > 0.05 else -1 for g in gx], np.int64)
        bwd = np.array([rs.randint(x_off[g], x_off[g + 1]) if x_off[g + 1] > x_off[g] and rs.rand() > 0.05 else -1 for g in gy], np.int64)
        for i in np.nonzero((fwd >= 0) & (rs.rand(n_x) < 0.5))[0]:   # mutual best rows, for the intersection
            bwd[fwd[i]] = i
        fs = (rs.randint(0, 7, size=n_x) / np.float32(8)).astype(np.float32)
        bs = (rs.randint(0, 7, size=n_y) / np.float32(8)).astype(np.float32)
        fs[fwd < 0] = -np.inf
        bs[bwd < 0] = -np.inf
        ties = 0
        for threshold in (None, 0.25):
            a = gr.select_global(fwd, fs, bwd, bs, x_off, y_off, retrieval, threshold)
            b = gr.select_per_group(fwd, fs, bwd, bs, x_off, y_off, retrieval, threshold)
            assert mnr.as_triples(a[:3]) == mnr.as_triples(b[:3]) and np.array_equal(a[3], b[3])
            assert len(a[0]) > 20
            ties += int((np.diff(a[0]) == 0).sum())
        assert ties > 20


# ---- 5
@pytest.fixture(scope="module")
def example_refs():
    x, y = gr.example_rows(GD)
    refs = {}
    for storage in mr.STORAGES:
        refs["x_in_y", storage] = gr.example_reference(x, mr.round_storage(y.astype(np.float32), storage), storage)
        refs["y_in_x", storage] = gr.example_reference(y, mr.round_storage(x.astype(np.float32), storage), storage)
    return refs


@pytest.mark.parametrize("storage", mr.STORAGES)
@pytest.mark.parametrize("direction", ["x_in_y", "y_in_x"])
def test_example_cuts_ambiguous_share(direction, storage, example_refs):
    ref = example_refs[direction, storage]
    worst = 0.0
    for cut, (xe, ye) in gr.EXAMPLE_CUTS.items():
        qe, de = (xe, ye) if direction == "x_in_y" else (ye, xe)
        for g in range(len(qe) - 1):
            e = gr.block_bound(ref, qe[g], qe[g + 1], de[g], de[g + 1])
            share = sr.ambiguous_share(ref["S64"][qe[g]:qe[g + 1], de[g]:de[g + 1]], K, e)
            print("%s %s cut %s group %d: e %.3e, ambiguous positions %.4f" % (direction, storage, cut, g, e, share))
            worst = max(worst, share)
            assert share <= sr.AMBIGUOUS_CAP
    assert worst > 0   # the exemption is not empty: the rule is exercised


def test_block_bound_is_rows_search_reference(example_refs):
    x, y = gr.example_rows(GD)
    (xe, ye) = gr.EXAMPLE_CUTS["three"]
    for storage in mr.STORAGES:
        db = mr.round_storage(y.astype(np.float32), storage)
        want = sr.rows_search_reference(x[xe[1]:xe[2]].astype(np.float32), db[ye[1]:ye[2]], storage)
        ref = example_refs["x_in_y", storage]
        assert gr.block_bound(ref, xe[1], xe[2], ye[1], ye[2]) == want["e"]
        assert np.array_equal(ref["S64"][xe[1]:xe[2], ye[1]:ye[2]], want["S64"])


# ---- 6
def test_plan_batches():
    from svx.postprocess.mine_local import plan_batches
    counts = [(5, 7), (3, 3), (9, 1), (1, 9), (30, 2), (2, 2), (2, 2)]
    batches = plan_batches(counts, 10)
    assert [i for b in batches for i in b] == list(range(len(counts)))       # every pair once, in order
    assert batches == [[0, 1], [2, 3], [4], [5, 6]]                            # a pair above the limit stands alone
    for b in batches:
        if len(b) > 1:
            assert sum(counts[i][0] for i in b) <= 10 and sum(counts[i][1] for i in b) <= 10
    assert plan_batches([], 10) == [] and plan_batches(counts, 1000) == [list(range(len(counts)))]


def _tree(tmp_path, docs):
    """docs: {stem: (rows in the embed file, candidate lines)} per language; -> metadata path."""
    for lang in ("en", "de"):
        (tmp_path / "cat" / lang).mkdir(parents=True)
        (tmp_path / "emb" / lang).mkdir(parents=True)
    meta = []
    for i, ((ns, ls), (nt, lt)) in enumerate(docs):
        for lang, rows, lines in (("en", ns, ls), ("de", nt, lt)):
            np.full((rows, 1024), 1.0, np.float16).tofile(tmp_path / "emb" / lang / f"doc{i}_{lang}.embed")
            (tmp_path / "cat" / lang / f"doc{i}_{lang}.txt").write_text("".join(f"{j} {j + 1}\n" for j in range(lines)))
        meta.append(f"/audio/doc{i}_en.wav\t/audio/doc{i}_de.wav")
    meta.append("/audio/missing_en.wav\t/audio/missing_de.wav")
    (tmp_path / "meta.tsv").write_text("\n".join(meta) + "\n")
    return tmp_path / "meta.tsv"


def test_cli_host_logic(tmp_path):
    from pathlib import Path
    from svx.postprocess import mine_local as ml
    from svx.utils.file_utils import read_metadata
    docs = [((20, 20), (18, 18)), ((7, 7), (30, 30)), ((25, 24), (25, 25)), ((40, 40), (41, 41)), ((16, 16), (16, 16))]
    meta = _tree(tmp_path, docs)
    pairs = ml.resolve_pairs(read_metadata(meta), tmp_path / "cat" / "en", tmp_path / "cat" / "de", tmp_path / "emb" / "en",
                             tmp_path / "emb" / "de", tmp_path / "out")
    assert len(pairs) == 5                                     # the pair without files is dropped
    assert [Path(p.output_path).name for p in pairs] == [f"doc{i}_en-doc{i}_de.txt" for i in range(5)]
    # shards of --n_shard 2 partition the pair list
    shards = [ml.shard_pairs(pairs, 2, r) for r in range(2)]
    assert sorted(p.output_path for s in shards for p in s) == sorted(p.output_path for p in pairs)
    assert all(shards) and not {p.output_path for p in shards[0]} & {p.output_path for p in shards[1]}
    assert ml.shard_pairs(pairs, 1, 0) == pairs
    # rows and lines; a count mismatch is skipped
    lines = [ml.count_rows(p, False, True) for p in pairs]
    assert [(p.n_src, p.n_tgt) for p in pairs] == [(20, 18), (7, 30), (25, 25), (40, 41), (16, 16)]
    assert lines[2] is None and all(l is not None for i, l in enumerate(lines) if i != 2)
    assert lines[0][0][:2] == ["0 1", "1 2"] and len(lines[0][1]) == 18
    # groups -> batches under --batch_rows
    ready = [p for p, l in zip(pairs, lines) if l is not None and p.n_src >= 16 and p.n_tgt >= 16]
    assert [Path(p.output_path).name[:4] for p in ready] == ["doc0", "doc3", "doc4"]
    assert ml.plan_batches([(p.n_src, p.n_tgt) for p in ready], 60) == [[0, 1], [2]]
    a = ml.parse_args([str(meta), str(tmp_path / "out"), "--src_lang", "en", "--tgt_lang", "de", "--concat_dir", "c", "--embed_dir", "e"])
    assert (a.k, a.margin, a.retrieval, a.threshold, a.batch_rows, a.skip_existing) == (16, "ratio", "max", None, ml.DEFAULT_BATCH_ROWS, False)
