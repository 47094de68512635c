"""Every Python entry that reaches the device, and the C ABI's svx_set_stream, on a torch side stream.

The rest of the suite runs svx on torch's default stream (the legacy null stream, handle 0), where a launch on the
wrong stream and a missing order between two bindings cannot show.  Here every entry is called under
`with torch.cuda.stream(s)` behind a delayed producer (tests/stream_probe.py): its device inputs hold a valid decoy data
set, the copy of the real data is queued behind a spin on `s`, and the entry is called at once.  Expected values are
the same entry's null-stream results, which other test files pin against float64 references; every comparison is bit
for bit.  B5 changes stream between dependent calls with no synchronisation in between: the context carries state
(arena, post-processing scratch, the last run's planes, held-back halves), so svx_set_stream has to order the old
binding's work in front of the new one's.

Synchronous by design, so without the in-flight assertion (each such case passes synchronous=True where it is probed and
says why): run_widen and everything that returns host data -- prior_width, GivenScores.fetch, raw_results,
svx_debug_level, svx_copy_to_host, the per-op functions on host arrays, the CLI.  band_contact launches and returns
(svx_contact.hip), so it carries the assertion like every other asynchronous entry.

Not covered: a missing join of an internal stream (side, helper, chain) back into the caller's stream cannot be made
deterministic from outside; it shows here only as far as the bit-equality happens to catch it.

Hand-run on the GPU box:
    python tests/test_gpu_stream_order.py --dump FILE
runs the file and writes one JSON line per probed case with the measured host time, the delay it chose and whether the
delay was in flight when the entry returned (profiles/stream_order.jsonl); no assertion refers to those values."""
import ctypes
import json
import os
import sys
import time

import numpy as np
import pytest

if __name__ == "__main__":   # hand-run: the paths conftest.py sets up for pytest
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_root, "speech-vecalign_amd"), os.path.join(_root, "oracle"), os.path.dirname(os.path.abspath(__file__))):
        sys.path.insert(0, _p)

import dp_ref
import stream_probe as sp
from synth import alignment_types, make_pair

pytestmark = pytest.mark.gpu
T5 = alignment_types(5)
TRIM = os.path.join(os.path.dirname(__file__), "golden", "example_trim")

# the search modes of PreparedBatch.run(): shapes and parameters of the smallest existing case of each family
#   name: (sizes, types, W, max_size_full_dp, search, blocks of the block prior)
MODES = {
    "coarse_to_fine": ([(300, 280), (211, 333), (120, 97), (402, 399)], T5, 7, 100, "coarse_to_fine", 0),   # dp_ref.Z_FUSED a5_W7_f32_ragged4
    "straight_narrow": ([(200, 190)], T5, 16, 0, "straight", 0),                                             # dp_ref.Z_STRAIGHT narrow_a5_W16
    "straight_wide": ([(150, 137), (70, 90), (40, 200)], T5, 40, 0, "straight", 0),                          # test_gpu_row_slack_wide.RAGGED
    "around": ([(120, 97)], T5, 7, 300, "around", 4),                                                        # test_gpu_around: 120 x 97, 4 blocks
    "around_wide": ([(120, 97)], T5, 33, 300, "around_wide", 4),                                             # test_gpu_around_wide: band of 66
}


@pytest.fixture(scope="module")
def streams():
    import torch
    from svx import _lib
    ctx = _lib.context()
    was = ctx.pipeline
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    yield s1, s2
    torch.cuda.synchronize()
    ctx = _lib.context()   # (back on the default stream)
    ctx.set_pipeline(was)
    ctx.sync()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def block_prior(n, m, cuts_x, cuts_y):
    """Prior rows [n + m + 2, 4] (zero padded) and info [2] of the blocks between the given cut fractions."""
    from svx.vecalign.dp_utils import prior_rows_from_alignments
    xs, ys = [int(n * c) for c in cuts_x], [int(m * c) for c in cuts_y]
    al = [(list(range(xs[i], xs[i + 1])), list(range(ys[i], ys[i + 1]))) for i in range(len(xs) - 1)]
    h = prior_rows_from_alignments(al)
    rows = np.zeros((n + m + 2, 4), np.int32)
    rows[:len(h)] = h
    return rows, np.array([len(h), 0], np.int32)


class Batch:
    """A PreparedBatch of one search mode, the device tensors its run() reads, and a real and a decoy data set for them."""

    def __init__(self, mode, time_prior=False, seed=0):
        from svx.vecalign import dp_utils
        sizes, types, W, max_full, search, blocks = MODES[mode]
        K = max(x for x, _ in types)
        docs = [make_pair(n, m, K, 32, seed=100 + seed + i, deletions=3) for i, (n, m) in enumerate(sizes)]
        other = [make_pair(n, m, K, 32, seed=200 + seed + i, deletions=5) for i, (n, m) in enumerate(sizes)]
        frames = [tuple(np.stack([16000 * np.arange(k), 16000 * np.arange(k) + 12000], axis=1) for k in nm) for nm in sizes]
        kw, pri_real, pri_decoy = {}, [], []
        if blocks:
            even = [i / blocks for i in range(blocks + 1)]
            for n, m in sizes:
                pri_real.append(block_prior(n, m, even, even))
                pri_decoy.append(block_prior(n, m, [0, 0.2, 0.6, 1], [0, 0.4, 0.7, 1]))   # (other slants: another covering width)
            kw["priors"] = [None] * len(sizes) if time_prior else [(dev(r), dev(i)) for r, i in pri_real]
        self.pb = dp_utils.PreparedBatch([(dev(a), dev(b)) for a, b in docs], types, dp_ref.FRAC, W, max_full, dp_ref.SAMPLE, dp_ref.NSAMP,
                                         rngs=[np.random.RandomState(900 + i) for i in range(len(sizes))], search=search, frames=frames, **kw)
        self.tensors = [v for ab in self.pb.vecs for v in ab]
        self.real = [dev(v) for ab in docs for v in ab]
        self.decoy = [dev(v) for ab in other for v in ab]
        if blocks and not time_prior:
            self.tensors += [v for ri in kw["priors"] for v in ri]
            self.real += [dev(v) for ri in pri_real for v in ri]
            self.decoy += [dev(v) for ri in pri_decoy for v in ri]

    def fill_real(self):
        for t, s in zip(self.tensors, self.real):
            t.copy_(s)

    def fill_decoy(self):
        for t, s in zip(self.tensors, self.decoy):
            t.copy_(s)

    def outputs(self):
        pb = self.pb
        return [pb.align, pb.scores, pb.info, pb.del_pen]

    def canon(self, arrs, extra=None):
        """The defined part of run()'s outputs (rows past a pair's count are whatever an earlier run left) + the extras."""
        pb = self.pb
        align, scores, info, pen = arrs[:4]
        out = [info, pen]
        for i in range(len(pb.vecs)):
            o, n = int(pb.offs[i]), max(0, int(info[i, 0]))
            out += [align[o:o + n], scores[o:o + n]]
        return out + (list(arrs[4:]) if extra is None else extra(arrs[4:], info))

    def check_ok(self, want):
        info = want[0]
        assert (info[:, 1] == 0).all() and (info[:, 0] > 0).all(), "the real data must align: %r" % info.tolist()


def with_pipeline(on):
    from svx import _lib
    ctx = _lib.context()
    ctx.set_pipeline(on)
    return ctx


# ---------------------------------------------------------------------------------------------- B2
@pytest.mark.parametrize("pipeline", [False, True], ids=["plain", "pipeline"])
@pytest.mark.parametrize("mode", list(MODES))
def test_run_behind_a_delayed_fill(streams, mode, pipeline):
    ctx = with_pipeline(pipeline)
    b = Batch(mode)

    def call():
        b.pb.run()
        if pipeline:
            b.pb.flush()
        return b.outputs()
    want = sp.probe_case("run[%s%s]" % (mode, ",pipeline" if pipeline else ""), streams[0], b.fill_real, b.fill_decoy, call, b.canon)
    b.check_ok(want)
    ctx.sync()


# ---------------------------------------------------------------------------------------------- B3
def rows_defined(arrs, info):
    """alignment_rows() / concat_rows(): only the first `count` rows are defined."""
    n = int(arrs[-1][0])
    return [a[:n] for a in arrs[:-1]] + [arrs[-1]]


def last_run_entries():
    def band_contact(b):
        return [b.pb.band_contact()]

    def own(b):
        g = b.pb.score_alignments(["own"] * len(b.pb.vecs))
        return [g.scores, g.total, g.report]

    def given(b):
        g = b.pb.score_alignments(b.given)
        return [g.scores, g.total, g.report]

    def slack(b):
        return list(b.pb.row_slack())

    def slack_wide(b):
        return list(b.pb.row_slack_wide())

    def alternatives(b):
        o = b.pb.row_alternatives(max_detour=8)
        return [o[k] for k in ("slack", "edge", "span", "summary", "detour", "detour_scores")]

    def align_rows(b):
        return list(b.pb.alignment_rows())

    def concat(b):
        return list(b.pb.concat_rows(dict(max_num_align=2)))

    def width(b):
        return [b.pb.prior_width_async()]
    #        name: (mode, entry, canon of the extras, entry comes before run(), synchronous)
    return {
        "band_contact": ("coarse_to_fine", band_contact, None, False, False),
        "score_alignments_own": ("coarse_to_fine", own, None, False, False),
        "score_alignments_given": ("coarse_to_fine", given, None, False, False),
        "row_slack": ("coarse_to_fine", slack, None, False, False),
        "row_slack_wide": ("straight_wide", slack_wide, None, False, False),
        "row_alternatives": ("straight_narrow", alternatives, None, False, False),
        "alignment_rows": ("coarse_to_fine", align_rows, rows_defined, False, False),
        "concat_rows": ("coarse_to_fine", concat, rows_defined, False, False),
        "prior_width_async": ("around_wide", width, None, True, False),
    }


@pytest.mark.parametrize("name", list(last_run_entries()))
def test_entries_that_read_the_last_run(streams, name):
    """run() followed by the entry, both behind the one delay."""
    mode, entry, extra, before, synchronous = last_run_entries()[name]
    ctx = with_pipeline(False)
    b = Batch(mode)
    if name == "score_alignments_given":   # the rows the real data aligns to: a valid given alignment for either data set
        b.fill_real()
        b.pb.run()
        info, align, _, _, offs = b.pb.raw_results()
        b.given = [align[int(offs[i]):int(offs[i]) + int(info[i, 0])].copy() for i in range(len(b.pb.vecs))]

    def call():
        if before:
            out = entry(b)
            b.pb.run()
        else:
            b.pb.run()
            out = entry(b)
        return b.outputs() + out
    want = sp.probe_case(name, streams[0], b.fill_real, b.fill_decoy, call, lambda a: b.canon(a, extra), synchronous)
    b.check_ok(want)
    ctx.sync()


def test_time_prior_then_run(streams):
    ctx = with_pipeline(False)
    b = Batch("around", time_prior=True)

    def call():
        b.pb.time_prior(20 * 16000, 8000)
        b.pb.run()
        return b.outputs() + [v for ri in b.pb.prior_own for v in ri]

    def canon(arrs):
        return b.canon(arrs, lambda extra, info: [extra[0][:max(0, int(extra[1][0]))], extra[1]])
    want = sp.probe_case("time_prior", streams[0], b.fill_real, b.fill_decoy, call, canon)
    b.check_ok(want)
    ctx.sync()


def test_run_widen(streams):
    """Synchronous by design; its report is host data."""
    ctx = with_pipeline(False)
    b = Batch("straight_narrow")

    def call():
        return b.outputs() + [dev(b.pb.run_widen(guard=2, max_rounds=1))]
    want = sp.probe_case("run_widen", streams[0], b.fill_real, b.fill_decoy, call, b.canon, synchronous=True)
    b.check_ok(want)
    ctx.sync()


# ---------------------------------------------------------------------------------------------- B4
# 64 queries, 257 rows, k = 4; the narrow width is 96, not 72: the k-NN and unit-row kernels take multiples of 32 only
# (svx_unit_rows answers d = 72 with SVX_ERR_ARG), and 96 is the smallest width above it that is no power of two.  The
# gather, which takes any multiple of 8, runs at 72.
N_Q, N_DB, KNN, D_NARROW = 64, 257, 4, 96
INDEX_SHAPES = [(D_NARROW, "fp16"), (D_NARROW, "bf16"), (1024, "fp16"), (1024, "bf16")]


def unit_data(n, d, seed):
    return np.random.RandomState(seed).randn(n, d).astype(np.float32)


class Index:
    """Two indexes built on the default stream -- the ordinary way to hold an index -- and query tensors with a real and a
    decoy data set."""

    def __init__(self, d, storage):
        import torch
        from svx.postprocess.flat_index import FlatIndex
        self.d, self.storage = d, storage
        self.x, self.y = FlatIndex(d, storage), FlatIndex(d, storage)
        self.x.add(unit_data(N_DB, d, 1))
        self.y.add(unit_data(N_DB - 57, d, 2))
        self.x.rows, self.y.rows
        self.empty = FlatIndex(d, storage)
        self.q, self.q2 = dev(unit_data(N_Q, d, 3)), dev(unit_data(N_Q, d, 4))
        self.real = [self.q.clone(), self.q2.clone()]
        self.decoy = [dev(unit_data(N_Q, d, 5)), dev(unit_data(N_Q, d, 6))]
        torch.cuda.synchronize()

    def fill_real(self):
        self.q.copy_(self.real[0]), self.q2.copy_(self.real[1])

    def fill_decoy(self):
        self.q.copy_(self.decoy[0]), self.q2.copy_(self.decoy[1])


def index_entries():
    def add(ix):
        ix.empty._chunks = []
        ix.empty.add(ix.q)
        return [ix.empty._chunks[0]]

    def mean_sim(ix):
        return [ix.x.mean_sim(ix.q, KNN)]

    def merge_topk(ix):
        topk, mean0 = ix.x.merge_topk(ix.q, KNN, want_mean=True)          # first
        first = topk.clone()
        topk, mean = ix.y.merge_topk(ix.q, KNN, topk, want_mean=True)     # merging
        return [first, mean0, topk, mean]

    def search(ix):
        return list(ix.x.search(ix.q, KNN))

    def search_l2(ix):
        return list(ix.x.search(ix.q, KNN, l2=True))

    def search_groups(ix):
        return list(ix.x.search_groups(ix.q, KNN, [0, 20, N_Q], [0, 100, N_DB]))

    def margin(ix):
        from svx.postprocess.score_align import margin_scores_device
        return [margin_scores_device(ix.x, ix.y, ix.q, ix.q2, KNN, "ratio")]
    return dict(add=add, mean_sim=mean_sim, merge_topk=merge_topk, search=search, search_l2=search_l2, search_groups=search_groups,
                margin_scores_device=margin)


@pytest.fixture(scope="module")
def indexes():
    made = {}

    def get(d, storage):
        if (d, storage) not in made:
            made[(d, storage)] = Index(d, storage)
        return made[(d, storage)]
    return get


@pytest.mark.parametrize("entry", list(index_entries()))
@pytest.mark.parametrize("d,storage", INDEX_SHAPES)
def test_index_built_on_the_default_stream_used_on_a_side_stream(streams, indexes, d, storage, entry):
    ix = indexes(d, storage)
    sp.probe_case("FlatIndex.%s[d%d,%s]" % (entry, d, storage), streams[0], ix.fill_real, ix.fill_decoy, lambda: index_entries()[entry](ix))


@pytest.mark.parametrize("entry", ["list_means", "candidate_scores"])
def test_mining_entries(streams, indexes, entry):
    import torch
    from svx.postprocess import mine
    ix = indexes(D_NARROW, "fp16")
    ix.fill_real()
    sets = []
    for q in (ix.real, ix.decoy):   # the searches' outputs, real and decoy, made on the default stream
        sims, ids = ix.x.search(q[0], KNN)
        sims_b, _ = ix.x.search(ix.x.rows, KNN)
        sets.append([sims.clone(), ids.clone(), mine.list_means(sims).clone(), (mine.list_means(sims_b) * (2 if q is ix.decoy else 1)).clone()])
    torch.cuda.synchronize()
    work = [t.clone() for t in sets[0]]

    def fill(k):
        return lambda: [w.copy_(s) for w, s in zip(work, sets[k])]

    def call():
        if entry == "list_means":
            return [mine.list_means(work[0])]
        best, score, scores = mine.candidate_scores(work[0], work[1], work[2], work[3], "ratio", want_scores=True)
        return [best, score, scores]
    sp.probe_case("mine.%s" % entry, streams[0], fill(0), fill(1), call)


@pytest.mark.parametrize("d,storage", INDEX_SHAPES)
def test_best_candidates(streams, d, storage):
    """The indexes' own rows are the entry's inputs: the fill rewrites them."""
    import torch
    from svx.postprocess import mine
    from svx.postprocess.flat_index import FlatIndex
    x, y = FlatIndex(d, storage), FlatIndex(d, storage)
    sets = []
    for seed in (10, 20):
        a, b = FlatIndex(d, storage), FlatIndex(d, storage)
        a.add(unit_data(N_DB, d, seed)), b.add(unit_data(N_DB - 57, d, seed + 1))
        sets.append([a.rows.clone(), b.rows.clone()])
    x.add_unit_rows(sets[0][0]), y.add_unit_rows(sets[0][1])
    work = [x.rows, y.rows]
    torch.cuda.synchronize()

    def fill(k):
        return lambda: [w.copy_(s) for w, s in zip(work, sets[k])]
    sp.probe_case("mine.best_candidates[d%d,%s]" % (d, storage), streams[0], fill(0), fill(1), lambda: list(mine.best_candidates(x, y, KNN, "ratio")))


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_gather_rows(streams, dt):
    import torch
    from svx.utils.embedding_utils import gather_candidates
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dt]
    real, decoy = dev(unit_data(N_DB, 72, 7)).to(tdt), dev(unit_data(N_DB, 72, 8)).to(tdt)
    emb = real.clone()
    table = dev(np.random.RandomState(9).randint(-1, N_DB, size=(4, 150)).astype(np.int32))   # (-1: a zero row)
    torch.cuda.synchronize()
    sp.probe_case("gather_candidates[%s]" % dt, streams[0], lambda: emb.copy_(real), lambda: emb.copy_(decoy), lambda: [gather_candidates(emb, table)])


# ---------------------------------------------------------------------------------------------- B1
def test_per_op_functions_on_device_tensors(streams):
    """make_norm1 (in place) and downsample_vectors take device tensors and stay on the device."""
    import torch
    from svx.vecalign import dp_utils
    from cases import OPS_CASE as c
    real = [dev(v) for v in make_pair(c["N"], c["M"], c["K"], c["d"], c["seed"])]
    decoy = [dev(v) for v in make_pair(c["N"], c["M"], c["K"], c["d"], c["seed"] + 1)]
    work = [t.clone() for t in real]
    torch.cuda.synchronize()

    def fill(src):
        return lambda: [w.copy_(s) for w, s in zip(work, src)]

    def call():
        dp_utils.make_norm1(work[0])
        return [work[0], dp_utils.downsample_vectors(work[1])]
    sp.probe_case("make_norm1+downsample_vectors", streams[0], fill(real), fill(decoy), call)


def test_per_op_functions_on_host_arrays(streams):
    """The per-op functions that take and return host arrays upload, launch and read back on the current stream: behind a
    spin on the side stream they return what they return on the null stream.  (Their inputs never rest on the device, so
    there is nothing a decoy could stand in for; they synchronise by design.)"""
    import torch
    from svx.vecalign import dp_core, dp_utils
    from cases import OPS_CASE as c
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "ops.npz"))
    v0, v1 = make_pair(c["N"], c["M"], c["K"], c["d"], c["seed"])
    types = alignment_types(c["a"])

    def every_op():
        out = {}
        a, b = v0.copy(), v1.copy()
        dp_utils.make_norm1(a), dp_utils.make_norm1(b)
        out["make_norm1"], out["downsample_vectors"] = a, dp_utils.downsample_vectors(a)
        np.random.seed(c["norm_seed"])
        out["compute_norms"] = dp_utils.compute_norms(a, b, 100)
        np.random.seed(5)
        knob = dp_utils.make_del_knob(a[0], b[0], gold["n0"][0], gold["n1"][0], 2000)
        out["make_del_knob"] = np.array([knob.percentile_frac_to_del_penalty(0.2)])
        al = dp_utils.dense_traceback(gold["dense_bp"].astype(np.int32))
        out["dense_traceback"] = dp_utils.alignments_to_rows(al)
        out["make_search_path"] = np.array(dp_utils.make_search_path(al, 2 * c["N"] + 1, 2 * c["M"], upsample=True), np.int32)
        csum, xp, yp, bout = gold["sparse_csum"], gold["sparse_xp"].astype(np.int32), gold["sparse_yp"].astype(np.int32), gold["b_offset_out"]
        sal, ssc = dp_utils.sparse_traceback(csum, xp, yp, bout, c["N"], c["M"])
        rows = np.asarray(dp_utils.alignments_to_rows(sal), np.int32).reshape(-1, 4)
        out["sparse_traceback"], out["sparse_scores"] = rows, ssc
        bsum = dp_utils.sparse_dp_backward(gold["sparse_costs"], gold["b_offset"], types, c["sparse_pen"], c["N"], c["M"])
        out["sparse_dp_backward"] = bsum
        out["path_slack"] = dp_utils.path_slack(gold["sparse_costs"], gold["b_offset"], types, c["sparse_pen"], c["N"], c["M"], csum, bsum, rows)
        alt = dp_utils.path_alternatives(gold["sparse_costs"], gold["b_offset"], types, c["sparse_pen"], c["N"], c["M"], csum, bsum, xp, yp, rows)
        for k in sorted(alt):
            if isinstance(alt[k], np.ndarray):
                out["path_alternatives." + k] = alt[k]
        return out
    torch.cuda.synchronize()
    want, again = every_op(), every_op()
    torch.cuda.synchronize()
    for k in want:
        assert sp.same_bits([np.asarray(want[k])], [np.asarray(again[k])]), "%s: two null-stream runs differ" % k
    with torch.cuda.stream(streams[0]):
        sp.delay(streams[0], sp.MIN_DELAY_MS)
        got = every_op()
    streams[0].synchronize()
    assert sorted(got) == sorted(want)
    for k in want:
        assert sp.same_bits([np.asarray(got[k])], [np.asarray(want[k])]), "%s differs on the side stream" % k


# ---------------------------------------------------------------------------------------------- B5
def last_run_reads(b, before_third=lambda: None):
    """The three entries of B5 (a) / (b).  All three stage their descriptors through the context's two pinned buffers taken
    in turn (svxl_scratch_begin), so the third waits on the host until the first one's upload has left its buffer:
    before_third() is the last moment at which nothing has waited."""
    pb = b.pb
    slack, summary = pb.row_slack()
    g = pb.score_alignments(["own"] * len(pb.vecs))
    before_third()
    return [slack, summary, pb.band_contact(), g.scores, g.total, g.report]


@pytest.mark.parametrize("pipeline", [False, True], ids=["a_plain", "b_pipeline"])
def test_run_on_one_stream_reads_on_another(streams, pipeline):
    """(a) delay + fill + run() on s1, then -- no synchronisation -- row_slack(), band_contact() and score_alignments("own")
    under s2, read back on s2.  (b) with the pipeline on and flush() under s2; the batch's outputs read back on both.
    The delay must still be in flight when row_slack() and score_alignments() have been issued under s2 (and flush()
    before them in (b)): none of them waits on the host.  It is queried there and not behind band_contact(), the third
    user of the two pinned staging buffers, which waits for row_slack()'s upload and so for the spin (last_run_reads)."""
    import torch
    s1, s2 = streams
    ctx = with_pipeline(pipeline)
    b = Batch("coarse_to_fine")

    def null():
        b.pb.run()
        if pipeline:
            b.pb.flush()
        return b.outputs() + last_run_reads(b)
    want, host_ms = sp.on_null_stream(b.fill_real, null)
    again, _ = sp.on_null_stream(b.fill_real, null)
    want = b.canon(want)
    assert sp.same_bits(want, b.canon(again))
    b.check_ok(want)
    decoy, _ = sp.on_null_stream(b.fill_decoy, null)
    assert not sp.same_bits(want, b.canon(decoy))
    torch.cuda.synchronize()
    ms = sp.delay_for(host_ms)
    with torch.cuda.stream(s1):
        ev = sp.delay(s1, ms)
        b.fill_real()
        b.pb.run()
    with torch.cuda.stream(s2):
        if pipeline:
            b.pb.flush()
        seen = []
        reads = last_run_reads(b, lambda: seen.append(ev.query() is False))
        on2 = sp.to_host(s2, b.outputs() + reads)
    on1 = sp.to_host(s1, b.outputs())
    s2.synchronize()
    got2 = b.canon(sp.as_numpy(on2))
    s1.synchronize()
    got1 = b.canon(sp.as_numpy(on1))
    sp.record("stream_change[%s]" % ("pipeline" if pipeline else "plain"), host_ms, ms, seen[0], False)
    assert sp.same_bits(got2, want), "read on s2: not the null-stream result"
    assert sp.same_bits(got1, want[:len(got1)]), "the batch's outputs read on s1, where it ran: not the null-stream result"
    assert seen[0], "the %.0f ms delay was over when the entries under s2 had been issued: delay too short, case inconclusive" % ms
    ctx.sync()


def test_two_batches_alternate_between_two_streams(streams):
    """(c) two batches of different scratch size, alternately on s1 (behind a delay) and s2: the arena and the
    post-processing scratch are shared, so each call has to queue behind the one before, whatever stream that ran on.
    No in-flight assertion: the second run() waits on the host, by design, until the first one's descriptor upload has
    left the pinned buffer they share, and that upload sits behind the spin.  What stays open is the window in which the
    first batch still runs on s1 while the second is launched on s2.  (Before svx_set_stream ordered its bindings this
    was more than a wrong number: the second run() uploads its pair descriptors into the same device array (the half's
    `dpairs`) and lays its levels out in the same arena while the first batch's kernels, queued on the other stream, still
    read both, so those kernels follow the other batch's pointers and sizes; that code ended this case with an illegal
    memory access, profiles/README.md.  The order the library now keeps is what makes the case safe to run.)"""
    import torch
    s1, s2 = streams
    ctx = with_pipeline(False)
    big, small = Batch("coarse_to_fine"), Batch("straight_narrow", seed=50)

    def both():
        out = []
        for b in (big, small, big, small):
            b.pb.run()
            out.append(b.outputs() + list(b.pb.row_slack()))
        return out

    def fill(real):
        for b in (big, small):
            b.fill_real() if real else b.fill_decoy()

    def canon(parts):
        return [a for b, p in zip((big, small, big, small), parts) for a in b.canon(p)]

    def null(real):
        fill(real)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        parts = both()
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        return canon([[o.cpu().numpy() for o in p] for p in parts]), ms
    want, host_ms = null(True)
    again, host_ms2 = null(True)
    assert sp.same_bits(want, again)
    assert not sp.same_bits(want, null(False)[0])
    torch.cuda.synchronize()
    host = []
    host_ms = min(host_ms, host_ms2)
    ms = sp.delay_for(host_ms)
    ev = sp.delay(s1, ms)
    with torch.cuda.stream(s1):
        big.fill_real()
        small.fill_real()
    for k, b in enumerate((big, small, big, small)):
        s = (s1, s2)[k % 2]
        with torch.cuda.stream(s):
            b.pb.run()
            host.append(sp.to_host(s, b.outputs() + list(b.pb.row_slack())))
    in_flight = ev.query() is False
    s1.synchronize(), s2.synchronize()
    sp.record("alternating_batches", host_ms, ms, in_flight, True)   # (the host waits by design: see above)
    assert sp.same_bits(canon([sp.as_numpy(h) for h in host]), want)
    ctx.sync()


def test_search_on_s2_right_after_a_delayed_run_on_s1(streams, indexes):
    """(d) both results must be right.  The search's queries are filled behind a delay of s2's own, three times s1's: a
    search that went to s1 instead would start when s1's spin ends, long before its queries are there."""
    import torch
    s1, s2 = streams
    ctx = with_pipeline(False)
    b, ix = Batch("coarse_to_fine"), indexes(D_NARROW, "fp16")

    def null(real):
        (b.fill_real if real else b.fill_decoy)(), (ix.fill_real if real else ix.fill_decoy)()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b.pb.run()
        sims, ids = ix.x.search(ix.q, KNN)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        return b.canon([o.cpu().numpy() for o in b.outputs()]), [sims.cpu().numpy(), ids.cpu().numpy()], ms
    want_run, want_search, host_ms = null(True)
    decoy_run, decoy_search, _ = null(False)
    assert not sp.same_bits(want_run, decoy_run) and not sp.same_bits(want_search, decoy_search)
    torch.cuda.synchronize()
    ms = sp.delay_for(host_ms)
    with torch.cuda.stream(s1):
        ev1 = sp.delay(s1, ms)
        b.fill_real()
        b.pb.run()
        h_run = sp.to_host(s1, b.outputs())
    with torch.cuda.stream(s2):
        ev2 = sp.delay(s2, 3 * ms)
        ix.fill_real()
        h_search = sp.to_host(s2, list(ix.x.search(ix.q, KNN)))
    in_flight = ev1.query() is False and ev2.query() is False
    s1.synchronize(), s2.synchronize()
    sp.record("search_after_run[s1]", host_ms, ms, in_flight, False)
    sp.record("search_after_run[s2]", host_ms, 3 * ms, in_flight, False)
    assert sp.same_bits(b.canon(sp.as_numpy(h_run)), want_run)
    assert sp.same_bits(sp.as_numpy(h_search), want_search)
    assert in_flight, "delay too short: inconclusive"
    ctx.sync()


# ---------------------------------------------------------------------------------------------- B6
STAGES = ["pyr0", "pyrN", "pyr_aux", "knob_scoresN", "knob", "dense_costs", "dense_dp", "path", "band_costs0", "band_costsN", "band_dp0",
          "band_dpN", "traceback", "setup", "total", "knob_sort", "knob_scores0", "pyr1", "tiles", "traceback0", "path0", "tiles_bwd"]


def level0_view(ctx, pair=0):
    """svx_debug_level (synchronises) + svx_copy_to_host of the level's csum -> (n_align, path_len, csum bytes)."""
    from svx import _lib
    v = _lib.LevelView()
    ctx.check(ctx.lib.svx_debug_level(ctx.h, pair, 0, ctypes.byref(v)))
    A, B = v.path_len + 2, v.band
    csum = np.empty((A, B), np.float64)
    ctx.check(ctx.lib.svx_copy_to_host(ctx.h, ctypes.c_void_p(csum.ctypes.data), ctypes.c_void_p(v.a_b_csum), csum.nbytes))
    return int(v.n_align), int(v.path_len), csum


def test_c_abi_set_stream(streams):
    import torch
    from svx import _lib
    s1, _ = streams
    ctx = with_pipeline(False)
    lib, vp = ctx.lib, ctypes.c_void_p
    b = Batch("coarse_to_fine")
    pb = b.pb

    def align():
        ctx.check(lib.svx_align_batch(ctx.h, ctypes.byref(pb.prm), pb.cpairs, len(pb.vecs)))
    want, host_ms = sp.on_null_stream(b.fill_real, lambda: (align(), b.outputs())[1])
    want_view = level0_view(ctx)
    assert want_view[0] > 0 and want_view[1] > 2
    decoy, _ = sp.on_null_stream(b.fill_decoy, lambda: (align(), b.outputs())[1])
    decoy_view = level0_view(ctx)
    assert not sp.same_bits(b.canon(want), b.canon(decoy)) and not sp.same_bits([want_view[2]], [decoy_view[2]])
    torch.cuda.synchronize()
    try:
        # ---- a torch side stream's handle, the batch call, then the C ABI's own read-backs with no torch synchronisation
        ctx.check(lib.svx_set_stream(ctx.h, vp(s1.cuda_stream)))
        ms = sp.delay_for(host_ms)
        with torch.cuda.stream(s1):
            ev = sp.delay(s1, ms)
            b.fill_real()
        align()
        in_flight = ev.query() is False
        got_view = level0_view(ctx)
        sp.record("svx_set_stream+svx_align_batch", host_ms, ms, in_flight, False)
        assert got_view[:2] == want_view[:2] and sp.same_bits([got_view[2]], [want_view[2]])
        assert in_flight, "delay too short: inconclusive"
        got = sp.as_numpy(sp.to_host(s1, b.outputs()))
        s1.synchronize()
        assert sp.same_bits(b.canon(got), b.canon(want))
        # ---- NULL returns to the default stream: a call is not held up by a spin on the side stream
        ctx.check(lib.svx_set_stream(ctx.h, vp(0)))     # (the default stream now waits for what the context did on s1: all done)
        ev = sp.delay(s1, 50.0)
        align()
        ctx.check(lib.svx_synchronize(ctx.h))
        assert ev.query() is False, "after svx_set_stream(ctx, NULL) the call still ran behind the side stream's spin"
        assert sp.same_bits(b.canon([o.cpu().numpy() for o in b.outputs()]), b.canon(want))
        s1.synchronize()
        # ---- the same handle again is a no-op: nothing is launched, a held half stays held
        ctx.set_pipeline(True)
        ctx.check(lib.svx_set_profiling(ctx.h, 0))
        ctx.check(lib.svx_set_stream(ctx.h, vp(s1.cuda_stream)))
        align()   # four pairs, pipelined: the second half's chain is held back
        count = lambda: [lib.svx_stage_launches(ctx.h, s.encode()) for s in STAGES]
        before = count()
        assert min(before) >= 0
        for _ in range(2):
            ctx.check(lib.svx_set_stream(ctx.h, vp(s1.cuda_stream)))
        assert count() == before, "rebinding the bound stream launched something"
        ctx.check(lib.svx_set_stream(ctx.h, vp(0)))   # a change of stream flushes: the held chain is launched now
        assert sum(count()) > sum(before), "no half was held back: the no-op check above saw nothing"
        ctx.check(lib.svx_synchronize(ctx.h))
        assert sp.same_bits(b.canon([o.cpu().numpy() for o in b.outputs()]), b.canon(want))
    finally:
        lib.svx_set_stream(ctx.h, vp(0))
        lib.svx_synchronize(ctx.h)
        ctx.use_current_stream()
        ctx.set_pipeline(False)


# ---------------------------------------------------------------------------------------------- B7
def test_seg_align_cli_on_a_side_stream(streams, tmp_path):
    import torch
    from svx.seg_align import align as A
    from test_gpu_around import build_tree
    root = str(tmp_path / "data")
    build_tree(root)

    def run(out):
        A.main([os.path.join(root, "metadata.tsv"), out, "--src_lang", "en", "--tgt_lang", "de", "--seg_dir", os.path.join(root, "seg"),
                "--concat_dir", os.path.join(root, "cat"), "--embed_dir", os.path.join(root, "emb"),
                "--ign_indices_dir", os.path.join(root, "ign"), "--fp16_embed", "--seed", "3"])
        torch.cuda.synchronize()
        files = {}
        for d, _, names in os.walk(out):
            for n in names:
                with open(os.path.join(d, n), "rb") as f:
                    files[os.path.relpath(os.path.join(d, n), out)] = f.read()
        return files
    want = run(str(tmp_path / "out_default"))
    assert want and any(len(v) for v in want.values())
    with torch.cuda.stream(streams[0]):
        got = run(str(tmp_path / "out_side"))
    assert got == want


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", required=True)
    a = ap.parse_args()
    rc = pytest.main([os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider"])
    with open(a.dump, "w") as f:
        for r in sp.RECORDS:
            f.write(json.dumps(r) + "\n")
    print("%d cases, %d asynchronous ones with the delay over at return" % (
        len(sp.RECORDS), sum(1 for r in sp.RECORDS if not r["synchronous_by_design"] and not r["in_flight_at_return"])))
    sys.exit(int(rc))
