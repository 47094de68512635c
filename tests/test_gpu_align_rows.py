"""svx_alignment_rows on the GPU, driven through the C ABI on synthetic descriptors (align_rows_ref: rows, scores and info
are written into device tensors by the test, the aligner does not run), every output compared bit for bit with the numpy
restatement of the contract: count, src, the raw copies, the unit rows in fp16 and bf16 -- and the memory that must stay
untouched (rows >= min(count, cap) and a guard region behind every buffer keep their fill pattern).  One test runs it
behind a real PreparedBatch.run(), with the software pipeline off and on."""
import ctypes

import numpy as np
import pytest

import align_rows_ref as R

pytestmark = pytest.mark.gpu

CODES = {"f32": 0, "f16": 1, "bf16": 2}
ESIZE = {"f32": 4, "f16": 2, "bf16": 2}
GUARD = 4   # rows of fill pattern behind every output buffer


def _vp(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


class Device:
    """A batch of align_rows_ref on the device: one upload per kind of array, svx_pair records pointing into them."""

    def __init__(self, batch):
        import torch
        from svx import _lib
        self.ctx = _lib.context()
        self.ctx.use_current_stream()
        self.batch, self.torch = batch, torch
        pairs = batch["pairs"]
        up = lambda arrs: torch.from_numpy(np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in arrs])).to(self.ctx.tdev)
        self.bufs = [up([p[key] for p in pairs]) for key in ("v0", "v1", "align", "scores", "info")]
        self.cpairs = (_lib.Pair * len(pairs))()
        at = [b.data_ptr() for b in self.bufs]
        for c, p in zip(self.cpairs, pairs):
            c.vecs0, c.vecs1, c.align, c.scores, c.info = at
            c.k0, c.n = p["v0"].shape[:2]
            c.k1, c.m = p["v1"].shape[:2]
            at = [a + p[key].nbytes for a, key in zip(at, ("v0", "v1", "align", "scores", "info"))]

    def call(self, max_score, storage, cap, n_pairs=None, d=None, dtype=None, unit=(True, True)):
        """-> (rc, outputs as numpy byte arrays incl. the guard rows, count).  storage None: no unit rows."""
        t, ctx, b = self.torch, self.ctx, self.batch
        d = b["d"] if d is None else d
        e = ESIZE[b["dtype"]]
        mk = lambda row_bytes: t.full(((cap + GUARD) * row_bytes,), R.FILL, dtype=t.uint8, device=ctx.tdev)
        x_rows, y_rows, src = mk(d * e), mk(d * e), mk(8)
        x_unit = mk(d * 2) if storage is not None and unit[0] else None
        y_unit = mk(d * 2) if storage is not None and unit[1] else None
        count = t.full((1,), -1, dtype=t.int64, device=ctx.tdev)
        rc = ctx.lib.svx_alignment_rows(ctx.h, CODES[b["dtype"]] if dtype is None else dtype, d, self.cpairs,
                                        len(b["pairs"]) if n_pairs is None else n_pairs, float(max_score), cap,
                                        _vp(x_rows), _vp(y_rows), _vp(x_unit), _vp(y_unit), 2 if storage == "bf16" else 1, _vp(src), _vp(count))
        t.cuda.synchronize()
        out = dict(x_rows=x_rows, y_rows=y_rows, x_unit=x_unit, y_unit=y_unit, src=src)
        return rc, {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}, int(count.item())


def check(batch, ref, got, count, cap, storage):
    """Bit for bit: the first min(count, cap) rows equal the reference, every byte behind them is untouched."""
    assert count == ref["count"]
    w = min(count, cap)
    d, e = batch["d"], ESIZE[batch["dtype"]]
    for key, row_bytes, view in (("x_rows", d * e, ref["x_rows"].dtype), ("y_rows", d * e, ref["y_rows"].dtype), ("src", 8, np.int32),
                                 ("x_unit", d * 2, np.uint16), ("y_unit", d * 2, np.uint16)):
        if got[key] is None:
            assert storage is None and key.endswith("unit")
            continue
        buf = got[key]
        assert buf.size == (cap + GUARD) * row_bytes
        assert (buf[w * row_bytes:] == R.FILL).all(), "%s: memory behind row %d was written" % (key, w)
        have = buf[:w * row_bytes].view(view).reshape(w, row_bytes // np.dtype(view).itemsize)
        want = ref[key][:w]
        bad = np.nonzero((have != want).any(axis=1))[0]
        assert len(bad) == 0, "%s: %d of %d rows differ, first %d (src %s)" % (key, len(bad), w, bad[0], ref["src"][bad[0]])


_refs = {}


def fixture(name, storage):
    """Batch, device copy and reference of a case, built once per session and left unchanged."""
    if name not in _refs:
        batch = R.build(name)
        _refs[name] = (batch, Device(batch), {})
    batch, dev, refs = _refs[name]
    if storage not in refs:
        refs[storage] = R.reference(batch, batch["max_score"], storage)
    return batch, dev, refs[storage]


@pytest.mark.parametrize("storage", ["fp16", "bf16"])
@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("d", [32, 96, 1024])
def test_rows_and_unit_rows(d, dtype, storage):
    """Rows per pair 0, 1, 255, 256, 257, 513; a pair of deletions first, info[0] = 0 and a failed pair with out-of-range
    garbage in the middle and at the end; edge rows; scores at the threshold, one ulp above, NaN, +inf, -0.0."""
    batch, dev, ref = fixture("edges-d%d-%s" % (d, dtype), storage)
    cap = ref["count"] + 3
    rc, got, count = dev.call(batch["max_score"], storage, cap)
    assert rc == 0, dev.ctx.lib.svx_last_error(dev.ctx.h)
    check(batch, ref, got, count, cap, storage)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("d", [8, 2048])
def test_raw_rows_at_the_alignment_dimensions(d, dtype):
    batch, dev, ref = fixture("raw-d%d-%s" % (d, dtype), None)
    cap = ref["count"]
    rc, got, count = dev.call(batch["max_score"], None, cap)
    assert rc == 0, dev.ctx.lib.svx_last_error(dev.ctx.h)
    check(batch, ref, got, count, cap, None)


@pytest.mark.parametrize("name", ["rotation1", "rotation2", "one-pair", "tiny-pairs"])
def test_batch_shapes(name):
    """The pairs that keep nothing in the other two orders; a batch of one pair; 1500 pairs of 6 x 6 segments, whose chunk
    scan runs past one workgroup's width."""
    batch, dev, ref = fixture(name, "fp16")
    if name == "tiny-pairs":
        assert len(batch["pairs"]) == 1500 and ref["count"] > 1024
    cap = ref["count"]
    rc, got, count = dev.call(batch["max_score"], "fp16", cap)
    assert rc == 0, dev.ctx.lib.svx_last_error(dev.ctx.h)
    check(batch, ref, got, count, cap, "fp16")


def test_max_score_infinity_keeps_every_non_deletion():
    batch, dev, _ = fixture("edges-d32-f16", "fp16")
    ref = R.reference(batch, np.inf, "bf16")
    assert ref["count"] > R.reference(batch, batch["max_score"])["count"]
    rc, got, count = dev.call(np.inf, "bf16", ref["count"])
    assert rc == 0
    check(batch, ref, got, count, ref["count"], "bf16")


@pytest.mark.parametrize("short", ["one", "all"])
def test_capacity(short):
    """cap = total - 1 and cap = 0: count still reports the total, rows >= cap keep their fill pattern."""
    batch, dev, ref = fixture("edges-d96-bf16", "fp16")
    cap = ref["count"] - 1 if short == "one" else 0
    rc, got, count = dev.call(batch["max_score"], "fp16", cap)
    assert rc == 0, dev.ctx.lib.svx_last_error(dev.ctx.h)
    assert count == ref["count"] > cap
    check(batch, ref, got, count, cap, "fp16")


def test_no_pairs():
    batch, dev, ref = fixture("edges-d32-f32", "fp16")
    rc, got, count = dev.call(batch["max_score"], "fp16", 5, n_pairs=0)
    assert rc == 0 and count == 0
    assert all((v == R.FILL).all() for v in got.values())


def test_argument_errors_leave_the_stream_usable():
    from svx import _lib
    batch, dev, ref = fixture("edges-d32-f32", "fp16")
    T, cap = batch["max_score"], ref["count"]
    bad = [dict(d=24), dict(d=1056), dict(dtype=7), dict(unit=(True, False)), dict(unit=(False, True))]
    for kw in bad:
        rc, got, count = dev.call(T, "fp16", cap, **kw)
        assert rc == _lib.SVX_ERR_ARG, kw
        assert dev.ctx.lib.svx_last_error(dev.ctx.h).decode().startswith("svx_alignment_rows"), kw
        assert count == -1 and all(v is None or (v == R.FILL).all() for v in got.values()), kw   # nothing was queued
    rc, got, count = dev.call(T, None, cap, d=24)    # (without unit rows the alignment rule holds: 24 is a multiple of 8)
    assert rc == 0
    rc, got, count = dev.call(T, "fp16", cap)
    assert rc == 0
    check(batch, ref, got, count, cap, "fp16")


def test_scratch_is_the_contexts_own_and_counted():
    batch, dev, ref = fixture("tiny-pairs", "fp16")
    lib, h = dev.ctx.lib, dev.ctx.h
    rc, _, _ = dev.call(batch["max_score"], "fp16", ref["count"])
    assert rc == 0
    one = lib.svx_scratch_bytes(h)
    assert one >= 1500 * 64                      # the descriptor copy alone
    rc, _, _ = dev.call(batch["max_score"], "fp16", ref["count"])
    assert rc == 0 and lib.svx_scratch_bytes(h) == one   # grow-only, reused


def test_behind_a_real_run_with_and_without_the_pipeline():
    """Three ragged pairs with deletions, d = 256, f16: alignment_rows() equals the reference evaluated on the results read
    back, with the pipeline off and with it on and no explicit flush; the unit rows are what svx_unit_rows writes."""
    import torch
    from svx import _lib
    from svx.postprocess.flat_index import FlatIndex
    from svx.vecalign import dp_utils
    from synth import alignment_types, make_pair
    shapes = [(700, 650, 5), (330, 360, 9), (90, 70, 2)]
    docs = [make_pair(n, m, 4, 256, seed=40 + i, dtype=np.float16, deletions=dl, zero_rows=2) for i, (n, m, dl) in enumerate(shapes)]
    types = alignment_types(5)
    ctx = _lib.context()

    def run(max_score):
        pb = dp_utils.PreparedBatch(docs, types, 0.2, 7, 300, 20000, 100, rngs=[np.random.RandomState(7 + i) for i in range(len(docs))])
        pb.run()
        rows = pb.alignment_rows(max_score, "fp16")       # (no flush in between)
        n_kept = pb.rows_count()
        info, align, scores, _, offs = pb.raw_results()
        pairs = [dict(v0=docs[i][0], v1=docs[i][1], align=align[offs[i]:offs[i + 1]], scores=scores[offs[i]:offs[i + 1]], info=info[i])
                 for i in range(len(docs))]
        ref = R.reference(dict(pairs=pairs, d=256, dtype="f16"), max_score)
        assert n_kept == ref["count"] > 0
        x_rows, y_rows, x_unit, y_unit, src, count = rows
        assert x_rows.shape[0] == sum(min(n, m) for n, m, _ in shapes) >= n_kept
        assert np.array_equal(src[:n_kept].cpu().numpy(), ref["src"])
        for have, want in ((x_rows, ref["x_rows"]), (y_rows, ref["y_rows"])):
            assert np.array_equal(have[:n_kept].cpu().numpy().view(np.uint16), want)
        for raw, unit in ((x_rows, x_unit), (y_rows, y_unit)):
            idx = FlatIndex(256, "fp16")
            idx.add(raw[:n_kept])
            assert torch.equal(idx.rows.view(torch.int16), unit[:n_kept].view(torch.int16))
        live = np.concatenate([p["scores"][:p["info"][0]][(p["align"][:p["info"][0], 1] > 0) & (p["align"][:p["info"][0], 3] > 0)] for p in pairs])
        return ref, float(np.median(live))

    was = ctx.pipeline
    try:
        ctx.set_pipeline(False)
        everything, T = run(np.inf)
        some, _ = run(T)
        assert 0.2 * everything["count"] <= some["count"] <= 0.8 * everything["count"]
        ctx.set_pipeline(True)
        piped, _ = run(T)
    finally:
        ctx.set_pipeline(was)
    assert piped["count"] == some["count"] and np.array_equal(piped["src"], some["src"])
    assert np.array_equal(piped["x_rows"], some["x_rows"]) and np.array_equal(piped["y_rows"], some["y_rows"])
