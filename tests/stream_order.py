"""The stream-order protocol of include/nsdg.h, stated once (TEST INFRASTRUCTURE; tests/test_gpu_stream_order.py runs it on the device,
tests/test_stream_order_cpu.py holds its compare logic to a stand-in without one).

The header promises that a call is asynchronous on the context's stream: it reads what the stream has produced when the call's work
runs, not what memory held when the host made the call, and whatever is enqueued on the stream behind the call sees its results.  On the
null stream both hold by themselves.  On any other stream they hold only if every launch and copy of the call goes to that stream (or is
joined to it), so the protocol runs ONE call between a LATE PRODUCER and an EARLY CONSUMER on a side stream s:

  1. the work buffers W hold a decoy -- another valid, finite case --, the pure outputs hold SENTINEL;
  2. a bounded delay is enqueued on s;
  3. W.copy_(X_real) is enqueued on s, and the pure outputs are filled with SENTINEL on s once more (a call whose work ran ahead of the
     stream loses its result to that fill: calls without a device input are held to the order too);
  4. an event `gate` is recorded on s;
  5. the call is made on a context bound to s;
  6. right after it returns, gate.query(): False for an asynchronous call (the producer still runs -- a gate that has fired means the
     delay was too short and nothing was proven: the row FAILS), True for a call the header documents as host-blocking;
  7. O_seen = O.clone() is enqueued on s;
  8. W.copy_(X_decoy) is enqueued on s (a call whose work was still running somewhere else would read it);
  9. s is synchronised;
 10. O_seen must hold the bits of the same call made plainly -- inputs in place, a full synchronise before and after;
 11. host results are compared as values, and what a call must not write still holds SENTINEL.

The delay is ordinary device work that ends by itself; nothing here waits for a flag, for the host or for another stream."""
import time

SENTINEL = -7.0


class Case:
    """one call and its buffers.  call() makes the call and returns its host results (None: none); inputs: (work, real, decoy) triples of
    tensors of one shape -- the call reads (and, in place, writes) `work`; outputs: the tensors the call's results are read from (a `work`
    among them when the call is in place); fill: the outputs nothing but the call writes; setup(): the host-only setters the call relies on
    (grid, parameters, variant, mask: the contexts are shared by the rows); untouched(seen) -> the parts of the seen outputs the call must
    leave at SENTINEL; keep: whatever must outlive the case"""

    def __init__(self, call, inputs, outputs, fill=(), setup=None, untouched=None, keep=None):
        self.call, self.inputs, self.outputs, self.fill = call, list(inputs), list(outputs), list(fill)
        self.setup = setup or (lambda: None)
        self.untouched, self.keep = untouched, keep


class CudaBackend:
    """the stream operations of the protocol on a torch stream"""

    def __init__(self, torch, stream, delay):
        self.torch, self.stream, self._delay = torch, stream, delay

    def copy(self, dst, src):
        with self.torch.cuda.stream(self.stream):
            dst.copy_(src)

    def fill(self, t, value):
        with self.torch.cuda.stream(self.stream):
            t.fill_(value)

    def clone(self, t):
        with self.torch.cuda.stream(self.stream):
            return t.clone()

    def delay(self):
        with self.torch.cuda.stream(self.stream):
            self._delay()

    def record(self):
        e = self.torch.cuda.Event()
        e.record(self.stream)
        return e

    def synchronize(self):
        self.stream.synchronize()

    def synchronize_all(self):
        self.torch.cuda.synchronize()


def bits(t):
    """the tensor as integers of its width: equal bits, a NaN or a signed zero included"""
    import torch

    return t.view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[t.element_size()]) if t.is_floating_point() else t


def same_bits(a, b):
    import torch

    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def plain(case, backend):
    """the call made plainly: inputs in place, a full synchronise before and after.  (host results, clones of the outputs)"""
    backend.synchronize_all()
    case.setup()
    for w, real, _ in case.inputs:
        backend.copy(w, real)
    for o in case.fill:
        backend.fill(o, SENTINEL)
    backend.synchronize_all()
    host = case.call()
    backend.synchronize_all()
    seen = [backend.clone(o) for o in case.outputs]
    backend.synchronize_all()
    return host, seen


def between_producer_and_consumer(case, backend):
    """steps 1 to 9.  (host results, O_seen, whether the gate had fired when the call returned, host seconds of the call)"""
    backend.synchronize_all()
    case.setup()
    for w, _, decoy in case.inputs:  # 1
        backend.copy(w, decoy)
    for o in case.fill:
        backend.fill(o, SENTINEL)
    backend.synchronize_all()
    backend.delay()  # 2
    for w, real, _ in case.inputs:  # 3
        backend.copy(w, real)
    for o in case.fill:
        backend.fill(o, SENTINEL)
    gate = backend.record()  # 4
    t0 = time.perf_counter()
    host = case.call()  # 5
    seconds = time.perf_counter() - t0
    fired = bool(gate.query())  # 6
    seen = [backend.clone(o) for o in case.outputs]  # 7
    for w, _, decoy in case.inputs:  # 8
        backend.copy(w, decoy)
    backend.synchronize()  # 9
    return host, seen, fired, seconds


def compare(name, got, want, case=None):
    """steps 10 and 11 on (host results, seen outputs) pairs"""
    (host_got, seen_got), (host_want, seen_want) = got, want
    assert host_got == host_want, "%s: host results %r, the plain call gives %r" % (name, host_got, host_want)
    assert len(seen_got) == len(seen_want)
    for k, (a, b) in enumerate(zip(seen_got, seen_want)):
        assert same_bits(a, b), "%s: output %d differs from the plain call in %d of %d values" % (
            name, k, int((bits(a) != bits(b)).sum()) if a.shape == b.shape else -1, a.numel())
    if case is not None and case.untouched is not None:
        for k, part in enumerate(case.untouched(seen_got)):
            assert bool((part == SENTINEL).all()), "%s: untouched part %d was written" % (name, k)


def check(name, case, backend, blocks_host, references):
    """the whole protocol for one row; references: the plain results the seen outputs must equal (side-stream context, default-stream
    context).  Returns the host seconds of the call"""
    host, seen, fired, seconds = between_producer_and_consumer(case, backend)
    if blocks_host:
        assert fired, "%s is documented as host-blocking but returned while the producer on its stream was still running" % name
    else:
        assert not fired, "%s: delay too short, nothing proven (the producer had finished when the call returned after %.3f ms)" % (name, 1e3 * seconds)
    for ref in references:
        compare(name, (host, seen), ref, case)
    return seconds
