"""Context.set_pipeline must not release held batches while their second-half chain is still queued: svx_set_pipeline
flushes only on a change of state, so set_pipeline(True) while already on (every call of it in a suite run with
SVX_PIPELINE=1) has to flush first, or keep the batches.  CPU only, with a stub library that records calls: freeing
tensors under a pending chain on a GPU would be running kernels on freed memory on purpose."""
from svx import _lib
from svx.vecalign import dp_utils


class StubLib:
    def __init__(self, align_rc=0):
        self.calls, self.align_rc = [], align_rc

    def __getattr__(self, name):   # every svx_* entry point: record the call, succeed
        def call(*args):
            self.calls.append(name)
            return self.align_rc if name == "svx_align_batch" else (b"stub failure" if name == "svx_last_error" else 0)
        return call


def stub_context(**kw):
    ctx = _lib.Context.__new__(_lib.Context)
    ctx.lib, ctx.h, ctx.device, ctx._held, ctx.pipeline = StubLib(**kw), None, 0, [], True
    ctx.use_current_stream = lambda: None
    return ctx


def test_set_pipeline_same_state_keeps_or_flushes_held_batches():
    for on in (True, False):
        ctx, b = stub_context(), object()
        ctx.hold(b)
        assert ctx._held == [b]
        ctx.set_pipeline(on)
        assert ctx.pipeline is on
        # released only behind a flush that came before the switch (svx_set_pipeline to the same state does not flush)
        assert any(x is b for x in ctx._held) or ctx.lib.calls[0] in ("svx_flush", "svx_synchronize"), ctx.lib.calls


def test_set_pipeline_without_held_batches_does_not_flush():
    ctx = stub_context()
    ctx.set_pipeline(True)
    assert ctx.lib.calls == ["svx_set_pipeline"]


def test_run_holds_the_batch_even_when_the_call_fails():
    ctx = stub_context(align_rc=_lib.SVX_ERR_HIP)
    pb = dp_utils.PreparedBatch.__new__(dp_utils.PreparedBatch)
    pb.ctx, pb.prm, pb.cpairs, pb.vecs = ctx, _lib.AlignParams(), (_lib.Pair * 1)(), [None]
    try:
        pb.run()
        raised = False
    except _lib.SvxError:
        raised = True
    assert raised and ctx._held == [pb]
