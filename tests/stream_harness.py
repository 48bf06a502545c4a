"""Late inputs on a side stream: what makes the `stream` argument of a library call something a test can see.

Every test of the suite issues its calls on torch's current stream, and that is the default (null) stream unless a test
enters another.  On the null stream a blocking copy, a fill, a launch without a stream and the call's own stream all run
in one order, so work that a call does outside its `stream` argument passes every such test.  Here the inputs of a call
are made LATE on a side stream:

    with late(torch, (dst, src), ...):      # dst: the device tensors the call reads, src: device tensors with the values
        rearm()                             # optional: another delay, between chained calls
        ... library calls through classpro_amd.api, which passes torch.cuda.current_stream() ...

1. on the default stream every dst is filled with poison (bytes 0xA5 for 8- and 16-bit tensors: sequences, labels, counts;
   -1 for 32- and 64-bit ones: offsets, keys, marks), and the device is synchronised;
2. the side stream is made current: one torch.cuda.Stream() for the process -- torch's streams do not block on the null
   stream, nor it on them -- picked by `side_stream` so that it does not share a hardware queue with the null stream
   either (a process has a few hardware queues, streams are dealt onto them in turn, and two streams on one queue run
   one after the other whatever their flags);
3. on it a delay of DELAY_MS is queued, then dst.copy_(src) for every pair;
4. the body runs: work in the stream's order sees the values, work outside it (another stream, a blocking copy) runs at
   once, ten milliseconds early, and sees the poison or a table that was not written yet;
5. on exit the stream is synchronised.

The control: right after arming, a clone of the first dst is queued on the DEFAULT stream.  After the last synchronise
it must still be all poison: that is the proof that work on the default stream overtook the side stream in this very
arming.  When it is not, the delay was too short or the streams block each other, and the test fails with that message; it
never passes without having been able to see an escape.

The delay is torch.cuda._sleep(cycles).  The rate of the counter behind it is not assumed: `calibrate` times one sleep
with two events and scales it to DELAY_MS; `cycles_per_ms` is the measured rate.  Where _sleep is missing, or does not
wait, the delay is a chain of large sorts on the side stream, sized the same way.

A plain module: no conftest.py, no pytest settings."""
import contextlib

DELAY_MS = 10.0                 # the host issues a call's first work within tens of microseconds of entry: two orders over
POISON_BYTE = 0xA5
SORT_N = 1 << 22                # the fallback delay: sorts of this many int32

_cal = {}                       # "mode": "sleep" | "sort", "cycles_per_ms", "unit" (cycles or sorts per DELAY_MS), "unit_ms"
_state = {"stream": None, "side": None, "armings": 0}
_fodder = {}


def _timed(torch, stream, fn):
    """Milliseconds fn() takes on `stream`, by two events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record()
        fn()
        b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _sort_fodder(torch):
    if "x" not in _fodder:
        _fodder["x"] = torch.randint(0, 1 << 30, (SORT_N,), dtype=torch.int32, device="cuda:0")
    return _fodder["x"]


def calibrate(torch, force=False):
    """Measures the delay once (again with force=True) and returns the calibration: dict(mode, cycles_per_ms, unit,
    unit_ms).  Bounded: at most a dozen timed sleeps, none longer than about 40 ms."""
    if _cal and not force:
        return _cal
    s = torch.cuda.Stream()
    sleep = getattr(torch.cuda, "_sleep", None)
    cal = None
    if sleep is not None:
        c = 1_000_000
        _timed(torch, s, lambda: sleep(1000))                       # the first launch loads the kernel
        for _ in range(12):
            ms = _timed(torch, s, lambda: sleep(c))
            if ms >= 4.0 or c >= 1 << 40:
                break
            c *= 4
        if ms >= 4.0:                                              # long enough for the events to resolve it
            rate = c / ms
            cal = dict(mode="sleep", cycles_per_ms=rate, unit=int(rate * DELAY_MS), unit_ms=DELAY_MS)
    if cal is None:                                                # no _sleep, or one that does not wait
        x = _sort_fodder(torch)
        _timed(torch, s, lambda: torch.sort(x))
        ms = max(_timed(torch, s, lambda: [torch.sort(x) for _ in range(4)]) / 4, 1e-3)
        n = max(1, int(DELAY_MS / ms + 0.999))
        cal = dict(mode="sort", cycles_per_ms=float("nan"), unit=n, unit_ms=n * ms)
    _cal.clear()
    _cal.update(cal)
    return _cal


def side_stream(torch):
    """The side stream of the process: the first of up to 16 new streams on which a delay does not hold up the default
    stream (a sleep is queued on it, then one small kernel on the default stream: that kernel is done while the sleep still
    runs).  When none is found the last one is kept and the control of every block says so."""
    if _state.get("side") is not None:
        return _state["side"]
    default = torch.cuda.default_stream()
    x = torch.zeros(64, device="cuda:0")
    for _ in range(16):
        s = torch.cuda.Stream()
        done = torch.cuda.Event()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            _delay(torch)
            done.record()
        with torch.cuda.stream(default):
            x.add_(1)
        default.synchronize()
        free = not done.query()                                    # the default stream ran ahead of the sleep
        s.synchronize()
        _state["side"] = s
        if free:
            break
    return s


def _delay(torch):
    """Queues DELAY_MS of waiting on the current stream."""
    cal = calibrate(torch)
    if cal["mode"] == "sleep":
        torch.cuda._sleep(cal["unit"])
    else:
        x = _sort_fodder(torch)
        for _ in range(cal["unit"]):
            torch.sort(x)
    _state["armings"] += 1


def poison_of(torch, t):
    """The poison value of a tensor by its element size (see the file comment)."""
    return -1 if t.element_size() >= 4 else (POISON_BYTE if t.dtype == torch.uint8 else POISON_BYTE - 256 if t.element_size() == 1
                                             else (POISON_BYTE << 8 | POISON_BYTE) - 65536)


def armings():
    """How many delays were queued in this process."""
    return _state["armings"]


def rearm():
    """Another delay on the side stream of the `late` block that is open: what an asynchronous call has queued so far is
    late for the next call."""
    import torch
    if _state["stream"] is None:
        raise RuntimeError("rearm() outside a late() block")
    assert torch.cuda.current_stream() == _state["stream"], "the side stream of late() is no longer current"
    _delay(torch)


@contextlib.contextmanager
def late(torch, *pairs):
    """See the file comment.  Yields the side stream."""
    if not pairs:
        raise ValueError("late() needs at least one (dst, src) pair: the control clones the first dst")
    if _state["stream"] is not None:
        raise RuntimeError("late() blocks do not nest")
    for dst, src in pairs:
        if dst.shape != src.shape or dst.dtype != src.dtype or not dst.is_cuda or not src.is_cuda or dst.data_ptr() == src.data_ptr():
            raise ValueError("a pair is two device tensors of one shape and type that do not share memory")
    calibrate(torch)
    default = torch.cuda.default_stream()
    with torch.cuda.stream(default):
        for dst, _ in pairs:
            dst.view(-1).fill_(poison_of(torch, dst))
    torch.cuda.synchronize()
    side = side_stream(torch)
    _state["stream"] = side
    try:
        with torch.cuda.stream(side):
            _delay(torch)
            for dst, src in pairs:
                dst.copy_(src)
            with torch.cuda.stream(default):                       # the control: the default stream, now
                first = pairs[0][0]
                seen = first.clone()
            yield side
            side.synchronize()
    finally:
        _state["stream"] = None
        torch.cuda.synchronize()
    want = torch.full_like(seen, poison_of(torch, first))
    assert torch.equal(seen, want), (
        "stream_harness: the control clone on the default stream saw the late values: the delay of %.1f ms (%s) was too short "
        "or the side stream blocks on the default stream; this arming could not have seen an escape" % (DELAY_MS, _cal.get("mode")))
