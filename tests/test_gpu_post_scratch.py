"""The post-processing scratch of a context (csrc/svx_common.h: one grow-only device buffer, two pinned staging buffers
taken in turn) under its four users on ONE context: svx_time_prior, svx_alignment_rows, svx_knn_search_groups and
svx_concat_rows queued one behind the other with no synchronisation in between.  Every output buffer, guard rows included,
equals bit for bit what the same call writes on a context of its own; the counts equal the CPU references of the calls'
own test files.

The scratch a call needs, in bytes (descriptors, tables and work arrays, each rounded up to 256):
    1 time prior, pairs of 5 x 4 and 70 x 90 segments      1 024   the buffer is created
    2 alignment rows, edges-d32-f32 (9 pairs, 14 chunks)   1 536   grows (the buffer of step 1 has 25 % slack: 1 280)
    3 grouped search, 3 groups, 2 workgroups                 768   falls: reuse
    4 concat rows, rotation2 (5 317 alignment rows)     ~167 000   grows while step 3's pinned buffer may still upload
    5 alignment rows, tiny-pairs (1 500 pairs)           126 208   falls; its pinned buffer (108 032 uploaded) grows
    6 time prior again                                     1 024   falls
The figures are the layout's, not measured: the test only asserts that the buffer grows at two calls after the first, stays
at one or more, never shrinks, and is left alone by a second round."""
import ctypes

import numpy as np
import pytest

import group_search_ref as gr
from test_gpu_align_rows import CODES, GUARD
from test_gpu_align_rows import fixture as rows_fixture
from test_gpu_concat_rows import _cparams
from test_gpu_concat_rows import fixture as concat_fixture
from test_gpu_margin_matrix import make_index

pytestmark = pytest.mark.gpu

FILL = 0xA5
K, D = 4, 32
GROUPS = [(20, 30), (0, 10), (40, 25)]   # (queries, database rows); the second group is empty


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _frames(rs, n):
    starts = np.sort(rs.randint(0, 40000, size=n))
    return np.stack([starts, starts + 5], axis=1).astype(np.int32)


class Calls:
    """The inputs of the six calls on the device, uploaded once; queue(i, ctx) allocates step i's outputs, queues the
    call on ctx and returns the output tensors without waiting for anything."""

    def __init__(self):
        import torch
        from svx import _lib
        self.torch, self.lib = torch, _lib
        rs = np.random.RandomState(11)
        self.tp = [(torch.from_numpy(_frames(rs, n)).cuda(), torch.from_numpy(_frames(rs, m)).cuda()) for n, m in ((5, 4), (70, 90))]
        self.rows = {name: rows_fixture(name, "fp16") for name in ("edges-d32-f32", "tiny-pairs")}
        self.cat = concat_fixture("rotation2", "fp16")
        q, db, self.q_off, self.db_off, _ = gr.lattice_groups(GROUPS, D, K, 17, "shuffled")
        self.db = make_index(db, "fp16").rows
        self.q = torch.from_numpy(q).cuda()
        torch.cuda.synchronize()

    def _buf(self, rows, row_bytes):
        return self.torch.full(((rows + GUARD) * row_bytes,), FILL, dtype=self.torch.uint8, device="cuda")

    def time_prior(self, ctx):
        t, L = self.torch, self.lib
        n = len(self.tp)
        cp, cf, co = (L.Pair * n)(), (L.Frames * n)(), (L.Prior * n)()
        out = []
        for i, (f0, f1) in enumerate(self.tp):
            cap = len(f0) + len(f1)
            rows, info = self._buf(cap, 16), self._buf(0, 8)
            cp[i].n, cp[i].m = len(f0), len(f1)
            cf[i].src, cf[i].tgt = f0.data_ptr(), f1.data_ptr()
            co[i].rows, co[i].info, co[i].cap = rows.data_ptr(), info.data_ptr(), cap
            out += [rows, info]
        ctx.check(ctx.lib.svx_time_prior(ctx.h, cp, cf, n, 4000, 700, co))
        return out

    def alignment_rows(self, ctx, name):
        batch, dev, ref = self.rows[name]
        d, e, cap = batch["d"], 4 if batch["dtype"] == "f32" else 2, ref["count"] + 1
        out = [self._buf(cap, d * e), self._buf(cap, d * e), self._buf(cap, d * 2), self._buf(cap, d * 2), self._buf(cap, 8), self._buf(0, 8)]
        ctx.check(ctx.lib.svx_alignment_rows(ctx.h, CODES[batch["dtype"]], d, dev.cpairs, len(batch["pairs"]), float(batch["max_score"]), cap,
                                             *[_vp(o) for o in out[:4]], 1, _vp(out[4]), _vp(out[5])))
        return out

    def concat_rows(self, ctx):
        from concat_rows_ref import PARAMS
        batch, dev, ref = self.cat
        d, e, cap = batch["d"], 4 if batch["dtype"] == "f32" else 2, ref["count"] + 1
        out = [self._buf(cap, d * e), self._buf(cap, d * e), self._buf(cap, d * 2), self._buf(cap, d * 2), self._buf(cap, 32), self._buf(0, 16)]
        ctx.check(ctx.lib.svx_concat_rows(ctx.h, CODES[batch["dtype"]], d, dev.cpairs, dev.cframes, len(batch["pairs"]), ctypes.byref(_cparams(PARAMS)),
                                          cap, *[_vp(o) for o in out[:4]], 1, _vp(out[4]), _vp(out[5])))
        return out

    def search_groups(self, ctx):
        n = int(self.q_off[-1])
        out = [self._buf(n, 4 * K), self._buf(n, 8 * K)]
        ctx.check(ctx.lib.svx_knn_search_groups(ctx.h, _vp(self.q), self.lib.SVX_F32, _vp(self.db), self.lib.SVX_F16, D, K,
                                                ctypes.c_void_p(self.q_off.ctypes.data), ctypes.c_void_p(self.db_off.ctypes.data), len(GROUPS),
                                                _vp(out[0]), _vp(out[1])))
        return out

    def queue(self, i, ctx):
        return (self.time_prior, lambda c: self.alignment_rows(c, "edges-d32-f32"), self.search_groups, self.concat_rows,
                lambda c: self.alignment_rows(c, "tiny-pairs"), self.time_prior)[i](ctx)


def test_four_users_take_turns_on_one_context():
    import torch
    from svx import _lib
    calls = Calls()

    def fresh():
        c = _lib.Context(torch.cuda.current_device())
        c.use_current_stream()
        return c

    # what each call writes on a context of its own
    alone = []
    for i in range(6):
        c = fresh()
        alone.append(calls.queue(i, c))
        c.sync()
    # the six calls on one context, nothing waited for in between; then the same again
    ctx = fresh()
    assert ctx.lib.svx_scratch_bytes(ctx.h) == 0
    rounds, sizes = [], []
    for _ in range(2):
        outs = []
        for i in range(6):
            outs.append(calls.queue(i, ctx))
            sizes.append(int(ctx.lib.svx_scratch_bytes(ctx.h)))
        rounds.append(outs)
    ctx.sync()
    for r, outs in enumerate(rounds):
        for i, (got, want) in enumerate(zip(outs, alone)):
            for j, (g, w) in enumerate(zip(got, want)):
                assert torch.equal(g, w), "round %d, call %d, output %d differs from the call on a context of its own" % (r + 1, i + 1, j)
    # the counts are the references' (the rows behind them are compared in the calls' own test files)
    first = rounds[0]
    assert int(first[1][5][:8].view(torch.int64)[0]) == calls.rows["edges-d32-f32"][2]["count"] > 0
    assert int(first[4][5][:8].view(torch.int64)[0]) == calls.rows["tiny-pairs"][2]["count"] > 1024
    assert first[3][5][:16].view(torch.int64).tolist() == [calls.cat[2]["count"], calls.cat[2]["wide"]]
    assert first[0][3][:8].view(torch.int32)[1] == 0 and first[0][3][:8].view(torch.int32)[0] > 2    # the 70 x 90 pair: rows, no failure
    assert (first[2][1][:8 * K * 20].view(torch.int64) >= 0).all()      # group 0 has k rows or more: every place is taken
    # the scratch: counted, grow-only, grown at two calls or more behind the first, reused at others, settled after one round
    one, two = sizes[:6], sizes[6:]
    assert one[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert sum(b > a for a, b in zip(one, one[1:])) >= 2 and sum(b == a for a, b in zip(one, one[1:])) >= 1
    assert two == [one[-1]] * 6
