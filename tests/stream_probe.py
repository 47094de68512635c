"""Stream-order probe; TEST INFRASTRUCTURE (torch and numpy only, no svx).

An entry that is "asynchronous on the current torch stream" must launch everything it does ON that stream.  The probe
makes a slip visible without any fault: the entry's device inputs hold DECOY data (a second valid data set of the same
shapes, dtypes and index ranges), a spin is put on the side stream, the copy of the REAL data into the same tensors is
queued behind the spin, and the entry is called at once.  Whatever the entry launches elsewhere runs while the spin
holds the fill back, reads the decoy and returns the decoy's result -- valid data, a wrong answer, a failed comparison.

The delay is no tolerance: it is what makes the probe sensitive, and cannot be derived.  A case measures the host time
of the entry's null-stream run and spins for max(20 ms, 4 x that); for an asynchronous entry the probe reports whether
the spin was still in flight when the entry returned, and the case asserts it ("delay too short: inconclusive" is then
told apart from a wrong result).  Used by test_gpu_stream_order.py."""
import time

import numpy as np

MIN_DELAY_MS = 20.0
HOST_FACTOR = 4.0      # host jitter on a shared machine
RECORDS = []           # one dict per probed case: host time, delay, in flight at return (test_gpu_stream_order.py --dump)

_cycles_per_ms = None
_mm = None             # (matrix, multiplications per ms) of the fallback spin


def _elapsed_ms(stream, work):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    work()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def _calibrate(stream):
    """Once per process: cycles of torch.cuda._sleep per millisecond, from two timing events around a fixed cycle count;
    a loop of large torch.mm sized the same way when _sleep is unusable."""
    global _cycles_per_ms, _mm
    import torch
    if _cycles_per_ms is not None or _mm is not None:
        return
    cycles = 20_000_000
    try:
        with torch.cuda.stream(stream):
            torch.cuda._sleep(1000)   # (first launch: module load)
            ms = _elapsed_ms(stream, lambda: torch.cuda._sleep(cycles))
        if ms > 0.5:
            _cycles_per_ms = cycles / ms
            return
    except Exception:
        pass
    with torch.cuda.stream(stream):
        m = torch.ones((2048, 2048), dtype=torch.float32, device="cuda")
        torch.mm(m, m)
        reps = 20

        def loop():
            for _ in range(reps):
                torch.mm(m, m)
        ms = _elapsed_ms(stream, loop)
    _mm = (m, reps / max(ms, 1e-3))


def delay(stream, ms):
    """A spin of at least `ms` milliseconds on `stream` -> the event recorded right behind it."""
    import torch
    _calibrate(stream)
    with torch.cuda.stream(stream):
        if _cycles_per_ms is not None:
            left = int(1.25 * ms * _cycles_per_ms) + 1   # (a quarter more: the clock the calibration saw may have been a slow one)
            while left > 0:   # (one launch takes a 32-bit cycle count on some builds)
                torch.cuda._sleep(min(left, 1 << 30))
                left -= 1 << 30
        else:
            m, per_ms = _mm
            for _ in range(int(1.25 * ms * per_ms) + 1):
                torch.mm(m, m)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def delay_for(host_ms):
    return max(MIN_DELAY_MS, HOST_FACTOR * host_ms)


def to_host(stream, outs):
    """Non-blocking copies of the device tensors `outs` to pinned host memory, queued on `stream` -> the pinned tensors
    (complete once the stream is synchronised)."""
    import torch
    host = []
    with torch.cuda.stream(stream):
        for o in outs:
            h = torch.empty(o.shape, dtype=o.dtype, pin_memory=True)
            h.copy_(o, non_blocking=True)
            host.append(h)
    return host


def as_numpy(host):
    """Pinned tensors -> numpy arrays of their bytes' own type (bf16 as uint16: numpy has no such type)."""
    import torch
    return [(h.view(torch.int16) if h.dtype == torch.bfloat16 else h).numpy().copy() for h in host]


def behind_delay(stream, fill, call, ms):
    """The probe.  The caller has filled the entry's device inputs with decoy data and called torch.cuda.synchronize().
    fill(): copy_ the real data into the same tensors; call(): the entry, -> list of device tensors (its outputs).
    -> (outputs as numpy arrays, was the delay's event still unfinished when call() returned)."""
    import torch
    with torch.cuda.stream(stream):
        ev = delay(stream, ms)
        fill()
        outs = call()
        in_flight = ev.query() is False
        host = to_host(stream, outs)
    stream.synchronize()
    return as_numpy(host), in_flight


def on_null_stream(fill, call):
    """The entry in the ordinary way, torch.cuda.synchronize() on both sides -> (outputs as numpy arrays, host wall time
    in ms of call() and the synchronisation behind it)."""
    import torch
    fill()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = call()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    host = to_host(torch.cuda.current_stream(), outs)
    torch.cuda.synchronize()
    return as_numpy(host), ms


def same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def record(case, host_ms, delay_ms, in_flight, synchronous):
    RECORDS.append(dict(case=case, host_ms=round(float(host_ms), 3), delay_ms=round(float(delay_ms), 3),
                        in_flight_at_return=bool(in_flight), synchronous_by_design=bool(synchronous)))


def probe_case(case, stream, fill_real, fill_decoy, call, canon=None, synchronous=False):
    """One probed case, the whole protocol: the entry twice on the null stream with the real data (bit-equal, or the
    entry is non-deterministic and the case says so), once with the decoy (must differ, or the case cannot fail), then --
    decoy still in the tensors, device idle -- behind the delay on `stream`, compared bit for bit.
    canon(arrays) -> arrays: cut the outputs down to their defined part (rows past a count hold whatever an earlier call
    left).  synchronous: the entry waits for the device by design, so the in-flight assertion does not apply.
    -> the expected arrays."""
    import torch
    canon = canon or (lambda a: a)
    want, host_ms = on_null_stream(fill_real, call)
    again, host_ms2 = on_null_stream(fill_real, call)
    want, again = canon(want), canon(again)
    assert same_bits(want, again), "%s: two null-stream runs differ (the entry is not deterministic; no stream finding)" % case
    decoy, _ = on_null_stream(fill_decoy, call)
    assert not same_bits(want, canon(decoy)), "%s: the decoy gives the real result: the case cannot fail, choose other seeds" % case
    torch.cuda.synchronize()
    ms = delay_for(min(host_ms, host_ms2))
    got, in_flight = behind_delay(stream, fill_real, call, ms)
    record(case, min(host_ms, host_ms2), ms, in_flight, synchronous)
    assert same_bits(canon(got), want), "%s: not the null-stream result: something ran outside the caller's stream" % case
    if not synchronous:
        assert in_flight, "%s: the %.0f ms delay was over when the entry returned: delay too short, case inconclusive" % (case, ms)
    return want
