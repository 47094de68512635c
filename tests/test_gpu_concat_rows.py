"""svx_concat_rows on the GPU, driven through the C ABI on synthetic descriptors (concat_rows_ref: rows, scores, info and
frames are written into device tensors by the test, the aligner does not run), every output compared bit for bit with the
restatement of the contract: counts, meta, the raw copies, the unit rows in fp16 and bf16 -- and the memory that must stay
untouched (rows >= min(count, cap) and a guard region behind every buffer keep their fill pattern).  One test runs it
behind a real PreparedBatch.run(), with the software pipeline off and on."""
import ctypes

import numpy as np
import pytest

import concat_rows_ref as C

pytestmark = pytest.mark.gpu

CODES = {"f32": 0, "f16": 1, "bf16": 2}
ESIZE = {"f32": 4, "f16": 2, "bf16": 2}
GUARD = 4   # rows of fill pattern behind every output buffer
KEYS = ("v0", "v1", "align", "scores", "info", "f0", "f1")


def _vp(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def _cparams(prm):
    from svx import _lib
    c = _lib.ConcatParams()
    c.max_score, c.max_num_align, c.sample_rate = float(prm["max_score"]), int(prm["max_num_align"]), int(prm["sample_rate"])
    c.max_sil, c.max_dur, c.both_sides, c.min_frames = float(prm["max_sil"]), float(prm["max_dur"]), int(prm["both_sides"]), int(prm["min_frames"])
    return c


class Device:
    """A batch of concat_rows_ref on the device: one upload per kind of array (every array padded to 16 bytes, the candidate
    tensors must be aligned), svx_pair and svx_frames records pointing into them."""

    def __init__(self, batch):
        import torch
        from svx import _lib
        self.ctx = _lib.context()
        self.ctx.use_current_stream()
        self.batch, self.torch = batch, torch
        pairs = batch["pairs"]
        pad = lambda a: np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.zeros(-a.nbytes % 16, np.uint8)])
        up = lambda arrs: torch.from_numpy(np.concatenate([pad(a) for a in arrs] + [np.zeros(16, np.uint8)])).to(self.ctx.tdev)
        self.bufs = [up([p[key] for p in pairs]) for key in KEYS]
        self.cpairs = (_lib.Pair * max(1, len(pairs)))()
        self.cframes = (_lib.Frames * max(1, len(pairs)))()
        at = [b.data_ptr() for b in self.bufs]
        for c, f, p in zip(self.cpairs, self.cframes, pairs):
            c.vecs0, c.vecs1, c.align, c.scores, c.info, f.src, f.tgt = at
            c.k0, c.n = p["v0"].shape[:2]
            c.k1, c.m = p["v1"].shape[:2]
            at = [a + p[key].nbytes + (-p[key].nbytes % 16) for a, key in zip(at, KEYS)]

    def call(self, prm, storage, cap, n_pairs=None, d=None, dtype=None, unit=(True, True), frames=True, entry="concat"):
        """-> (rc, outputs as numpy byte arrays incl. the guard rows, counts).  storage None: no unit rows.
        entry "align": svx_alignment_rows on the same batch (meta is then its src, [cap][2])."""
        t, ctx, b = self.torch, self.ctx, self.batch
        d = b["d"] if d is None else d
        e = ESIZE[b["dtype"]]
        mk = lambda row_bytes: t.full(((cap + GUARD) * row_bytes,), C.FILL, dtype=t.uint8, device=ctx.tdev)
        x_rows, y_rows, meta = mk(d * e), mk(d * e), mk(32 if entry == "concat" else 8)
        x_unit = mk(d * 2) if storage is not None and unit[0] else None
        y_unit = mk(d * 2) if storage is not None and unit[1] else None
        counts = t.full((2,), -1, dtype=t.int64, device=ctx.tdev)
        code = CODES[b["dtype"]] if dtype is None else dtype
        n_pairs = len(b["pairs"]) if n_pairs is None else n_pairs
        if entry == "concat":
            rc = ctx.lib.svx_concat_rows(ctx.h, code, d, self.cpairs, self.cframes if frames else None, n_pairs, ctypes.byref(_cparams(prm)), cap,
                                         _vp(x_rows), _vp(y_rows), _vp(x_unit), _vp(y_unit), 2 if storage == "bf16" else 1, _vp(meta), _vp(counts))
        else:
            rc = ctx.lib.svx_alignment_rows(ctx.h, code, d, self.cpairs, n_pairs, float(prm["max_score"]), cap,
                                            _vp(x_rows), _vp(y_rows), _vp(x_unit), _vp(y_unit), 2 if storage == "bf16" else 1, _vp(meta), _vp(counts))
        t.cuda.synchronize()
        out = dict(x_rows=x_rows, y_rows=y_rows, x_unit=x_unit, y_unit=y_unit, meta=meta)
        return rc, {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}, [int(v) for v in counts.cpu()]


def check(batch, ref, got, counts, cap, storage):
    """Bit for bit: the first min(count, cap) rows equal the reference, every byte behind them is untouched."""
    assert counts == [ref["count"], ref["wide"]]
    w = min(ref["count"], cap)
    d, e = batch["d"], ESIZE[batch["dtype"]]
    for key, row_bytes, view in (("meta", 32, np.int32), ("x_rows", d * e, ref["x_rows"].dtype), ("y_rows", d * e, ref["y_rows"].dtype),
                                 ("x_unit", d * 2, np.uint16), ("y_unit", d * 2, np.uint16)):
        if got[key] is None:
            assert storage is None and key.endswith("unit")
            continue
        buf = got[key]
        assert buf.size == (cap + GUARD) * row_bytes
        assert (buf[w * row_bytes:] == C.FILL).all(), "%s: memory behind row %d was written" % (key, w)
        have = buf[:w * row_bytes].view(view).reshape(w, row_bytes // np.dtype(view).itemsize)
        want = ref[key][:w]
        bad = np.nonzero((have != want).any(axis=1))[0]
        assert len(bad) == 0, "%s: %d of %d rows differ, first %d (meta %s)" % (key, len(bad), w, bad[0], ref["meta"][bad[0]])


_built = {}
_refs = {}


def fixture(name, storage, prm=C.PARAMS):
    """Batch, device copy and reference of a case, built once per session and left unchanged."""
    if name not in _built:
        batch = C.build(name)
        _built[name] = (batch, Device(batch))
    batch, dev = _built[name]
    key = (name, storage, tuple(sorted(prm.items())))
    if key not in _refs:
        _refs[key] = C.reference(batch, prm, storage)
    return batch, dev, _refs[key]


@pytest.mark.parametrize("storage", ["fp16", "bf16"])
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("d", [32, 96, 1024])
def test_rows_and_unit_rows(d, dtype, storage):
    """Pairs of 0, 1, 255, 256, 257, 513 and 1100 rows; pairs without base rows first, in the middle and last; runs over a
    chunk edge and over 300 rows that are no base rows; the equalities of max_dur, max_sil and min_frames; a pair edge
    that looks connected (test_concat_rows_cpu asserts that each of these is in the batch)."""
    batch, dev, ref = fixture("edges-d%d-%s" % (d, dtype), storage)
    cap = ref["count"] + 3
    rc, got, counts = dev.call(C.PARAMS, storage, cap)
    assert rc == 0, dev.ctx.lib.svx_last_error(dev.ctx.h)
    check(batch, ref, got, counts, cap, storage)


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("d", [8, 2048])
def test_raw_rows_at_the_alignment_dimensions(d, dtype):
    batch, dev, ref = fixture("raw-d%d-%s" % (d, dtype), None)
    cap = ref["count"]
    rc, got, counts = dev.call(C.PARAMS, None, cap)
    assert rc == 0, dev.ctx.lib.svx_last_error(dev.ctx.h)
    check(batch, ref, got, counts, cap, None)


@pytest.mark.parametrize("both", [0, 1])
@pytest.mark.parametrize("num", [1, 2, 3, 8])
def test_max_num_align_and_both_sides(num, both):
    prm = C.params(max_num_align=num, both_sides=both)
    batch, dev, ref = fixture("edges-d32-f16", "bf16", prm)
    if num == 8:
        assert (ref["meta"][:, 3] == 3).any() and ref["wide"] > ref["count"] // 8   # k = 3 x 3: what is longer is wide
    cap = ref["count"]
    rc, got, counts = dev.call(prm, "bf16", cap)
    assert rc == 0, dev.ctx.lib.svx_last_error(dev.ctx.h)
    check(batch, ref, got, counts, cap, "bf16")


@pytest.mark.parametrize("name", ["rotation1", "rotation2", "one-pair", "tiny-pairs", "no-rows"])
def test_batch_shapes(name):
    """The pairs without base rows in the other two orders (k = 4 x 2); a batch of one pair; 1500 tiny pairs, whose chunk
    scan runs past one workgroup's width; a batch that has no base row at all."""
    batch, dev, ref = fixture(name, "fp16")
    if name == "tiny-pairs":
        assert len(batch["pairs"]) == 1500 and ref["count"] > 1024
    if name == "no-rows":
        assert ref["count"] == 0
    cap = ref["count"] + 1
    rc, got, counts = dev.call(C.PARAMS, "fp16", cap)
    assert rc == 0, dev.ctx.lib.svx_last_error(dev.ctx.h)
    check(batch, ref, got, counts, cap, "fp16")


def test_no_duration_filter_and_no_cost_filter():
    prm = C.params(min_frames=0, max_score=np.inf)
    batch, dev, ref = fixture("edges-d32-f16", "fp16", prm)
    assert ref["count"] > fixture("edges-d32-f16", "fp16")[2]["count"]
    rc, got, counts = dev.call(prm, "fp16", ref["count"])
    assert rc == 0
    check(batch, ref, got, counts, ref["count"], "fp16")


@pytest.mark.parametrize("short", ["one", "half", "all"])
def test_capacity(short):
    """cap = total - 1, about half (the cut falls inside a workgroup's outputs and inside a run) and 0: counts still report
    the totals, rows >= cap keep their fill pattern."""
    batch, dev, ref = fixture("edges-d96-bf16", "fp16")
    cap = {"one": ref["count"] - 1, "half": ref["count"] // 2 + 1, "all": 0}[short]
    rc, got, counts = dev.call(C.PARAMS, "fp16", cap)
    assert rc == 0, dev.ctx.lib.svx_last_error(dev.ctx.h)
    assert counts[0] == ref["count"] > cap
    check(batch, ref, got, counts, cap, "fp16")


def test_no_pairs():
    batch, dev, ref = fixture("edges-d32-f32", "fp16")
    rc, got, counts = dev.call(C.PARAMS, "fp16", 5, n_pairs=0)
    assert rc == 0 and counts == [0, 0]
    assert all((v == C.FILL).all() for v in got.values())


@pytest.mark.parametrize("name,storage", [("edges-d96-f32", "fp16"), ("edges-d1024-bf16", "bf16"), ("raw-d2048-f16", None)])
def test_without_joining_it_is_svx_alignment_rows(name, storage):
    """max_num_align = 1, min_frames = 0, frames = NULL: the outputs of svx_alignment_rows on the same batch, bit for bit
    (k = 3 x 3 and every row of these batches is at most 2 x 2 wide, so its width limit drops nothing)."""
    prm = C.params(max_num_align=1, min_frames=0)
    batch, dev, ref = fixture(name, storage, prm)
    cap = ref["count"] + 2
    rc, got, counts = dev.call(prm, storage, cap, frames=False)
    assert rc == 0, dev.ctx.lib.svx_last_error(dev.ctx.h)
    check(batch, ref, got, counts, cap, storage)
    rc, old, old_count = dev.call(prm, storage, cap, entry="align")
    assert rc == 0 and old_count[0] == counts[0] > 0 and counts[1] == 0
    for key in ("x_rows", "y_rows", "x_unit", "y_unit"):
        assert (got[key] is None and old[key] is None) or np.array_equal(got[key], old[key]), key
    w = counts[0]
    assert np.array_equal(got["meta"][:w * 32].view(np.int32).reshape(w, 8)[:, :2], old["meta"][:w * 8].view(np.int32).reshape(w, 2))


def test_argument_errors_leave_the_stream_usable():
    from svx import _lib
    batch, dev, ref = fixture("edges-d32-f32", "fp16")
    cap = ref["count"]
    bad = [(C.params(max_num_align=0), {}), (C.params(max_num_align=9), {}), (C.PARAMS, dict(frames=False)),
           (C.params(max_num_align=1), dict(frames=False)),                      # (min_frames > 0 still needs the frames)
           (C.params(sample_rate=0), {}),
           (C.PARAMS, dict(d=24)), (C.PARAMS, dict(d=1056)), (C.PARAMS, dict(dtype=7)), (C.PARAMS, dict(unit=(True, False))),
           (C.PARAMS, dict(unit=(False, True)))]
    for prm, kw in bad:
        rc, got, counts = dev.call(prm, "fp16", cap, **kw)
        assert rc == _lib.SVX_ERR_ARG, (prm, kw)
        assert dev.ctx.lib.svx_last_error(dev.ctx.h).decode().startswith("svx_concat_rows"), kw
        assert counts == [-1, -1] and all(v is None or (v == C.FILL).all() for v in got.values()), kw   # nothing was queued
    rc, got, counts = dev.call(C.PARAMS, None, cap, d=24)    # (without unit rows the alignment rule holds: 24 is a multiple of 8)
    assert rc == 0
    rc, got, counts = dev.call(C.PARAMS, "fp16", cap)
    assert rc == 0
    check(batch, ref, got, counts, cap, "fp16")


def test_scratch_is_the_contexts_own_and_counted():
    batch, dev, ref = fixture("tiny-pairs", "fp16")
    lib, h = dev.ctx.lib, dev.ctx.h
    rc, _, _ = dev.call(C.PARAMS, "fp16", ref["count"])
    assert rc == 0
    one = lib.svx_scratch_bytes(h)
    assert one >= 1500 * 80                      # the descriptor copy alone
    rc, _, _ = dev.call(C.PARAMS, "fp16", ref["count"])
    assert rc == 0 and lib.svx_scratch_bytes(h) == one   # grow-only, reused


def test_behind_a_real_run_with_and_without_the_pipeline():
    """Three ragged pairs with deletions, d = 256, f16, made-up timestamps: concat_rows() equals the reference evaluated on
    the results read back, with the pipeline off and with it on and no explicit flush; the unit rows are what svx_unit_rows
    writes; fetch_async() brings counts and meta along."""
    import torch
    from svx import _lib
    from svx.postprocess.flat_index import FlatIndex
    from svx.vecalign import dp_utils
    from synth import alignment_types, make_pair
    shapes = [(700, 650, 5), (330, 360, 9), (90, 70, 2)]
    docs = [make_pair(n, m, 4, 256, seed=40 + i, dtype=np.float16, deletions=dl, zero_rows=2) for i, (n, m, dl) in enumerate(shapes)]
    frames = [(C.frames_for(np.random.RandomState(60 + i), n), C.frames_for(np.random.RandomState(80 + i), m)) for i, (n, m, _) in enumerate(shapes)]
    types = alignment_types(5)
    ctx = _lib.context()

    def run(max_score):
        prm = C.params(max_score=max_score)
        pb = dp_utils.PreparedBatch(docs, types, 0.2, 7, 300, 20000, 100, rngs=[np.random.RandomState(7 + i) for i in range(len(docs))], frames=frames)
        pb.run()
        rows = pb.concat_rows({k: v for k, v in prm.items()}, "fp16")       # (no flush in between)
        ev = pb.fetch_async()
        ev.synchronize()
        n_kept = pb.rows_count()
        info, align, scores, _, offs = pb.raw_results()
        pairs = [dict(v0=docs[i][0], v1=docs[i][1], align=align[offs[i]:offs[i + 1]], scores=scores[offs[i]:offs[i + 1]], info=info[i],
                      f0=frames[i][0], f1=frames[i][1]) for i in range(len(docs))]
        ref = C.reference(dict(pairs=pairs, d=256, dtype="f16"), prm)
        assert n_kept == ref["count"] > 0 and int(pb.h_rows[0][1]) == ref["wide"]
        x_rows, y_rows, x_unit, y_unit, meta, counts = rows
        assert x_rows.shape[0] == 3 * sum(min(n, m) for n, m, _ in shapes) >= n_kept
        assert np.array_equal(meta[:n_kept].cpu().numpy(), ref["meta"]) and np.array_equal(pb.h_rows[1].numpy()[:n_kept], ref["meta"])
        for have, want in ((x_rows, ref["x_rows"]), (y_rows, ref["y_rows"])):
            assert np.array_equal(have[:n_kept].cpu().numpy().view(np.uint16), want)
        for raw, unit in ((x_rows, x_unit), (y_rows, y_unit)):
            idx = FlatIndex(256, "fp16")
            idx.add(raw[:n_kept])
            assert torch.equal(idx.rows.view(torch.int16), unit[:n_kept].view(torch.int16))
        live = np.concatenate([p["scores"][:p["info"][0]][(p["align"][:p["info"][0], 1] > 0) & (p["align"][:p["info"][0], 3] > 0)] for p in pairs])
        return ref, float(np.quantile(live, 0.8))

    was = ctx.pipeline
    try:
        ctx.set_pipeline(False)
        everything, T = run(np.inf)
        assert (everything["meta"][:, 3] > 1).any() and everything["wide"] > 0
        some, _ = run(T)
        assert 0 < some["count"] < everything["count"]
        ctx.set_pipeline(True)
        piped, _ = run(T)
    finally:
        ctx.set_pipeline(was)
    assert piped["count"] == some["count"] and np.array_equal(piped["meta"], some["meta"])
    assert np.array_equal(piped["x_rows"], some["x_rows"]) and np.array_equal(piped["y_rows"], some["y_rows"])
