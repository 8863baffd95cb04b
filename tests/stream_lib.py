"""Late input on a busy stream: the one technique tests/test_gpu_caller_stream.py holds every `void *stream` entry point to.

A caller such as bench.py produces its inputs on a stream of its own immediately before the call and never drains the device in
between.  Here the stream S is kept busy for a calibrated delay (250 ms), the real input A is copied into place BEHIND the delay,
over a poison P -- another valid input of the same geometry whose correct answers differ --, the entry point is called on S, and its
outputs are copied out in stream order, with no synchronisation in between:

    dst <- P; out <- SENTINEL; device drained
    on S:  delay;  dst <- A;  entry point(stream = S);  keep <- out
    S drained;  keep must equal expected(A)

A step of the call that ran anywhere but on S runs during the delay: it reads P or the sentinel, or writes after `keep` was taken, so
the answer is wrong -- and nothing faults, since P is well-formed and offsets are never late.

The control (Late.control) is what gives this its power: the same set-up with the call on the library's OWN stream must return
expected(P).  If it returns expected(A), S and the context's stream share a hardware queue and are serialised by accident: the
caller takes another stream.  Test infrastructure only."""
import time

import numpy as np

TARGET_MS = 250.0
POISON_BYTE = 0x5A
SENTINEL32 = 0x5A5A5A5A

_VIEW = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}


def to_dev(torch, a, pad=0):
    """numpy array -> device tensor of the same bits (uint64 / uint32 as int64 / int32), `pad` zero elements appended"""
    a = np.ascontiguousarray(a)
    if pad:
        a = np.concatenate([a, np.zeros(pad, dtype=a.dtype)])
    v = _VIEW.get(a.dtype)
    return torch.from_numpy(a.view(v) if v else a).cuda()


def to_host(t, dtype):
    """device (or host) tensor -> numpy array of `dtype`, the same bits"""
    return np.ascontiguousarray(t.cpu().numpy()).view(dtype)


def sentinel(t):
    """every byte of a (contiguous) device tensor set to POISON_BYTE: SENTINEL32 in every 32-bit word"""
    import torch
    t.view(torch.uint8).fill_(POISON_BYTE)


class Delay:
    """Something that keeps a stream busy for about TARGET_MS: torch.cuda._sleep(cycles), or -- in a build without it -- a chain of
    large device copies.  Calibrated once, by timing it on a stream with events and scaling."""

    def __init__(self, torch, stream):
        self.torch = torch
        if hasattr(torch.cuda, "_sleep"):
            self.kind, self.n = "torch.cuda._sleep", 2_000_000
            self._buf = None
        else:
            self.kind, self.n = "copies of 256 MiB", 8
            self._buf = (torch.empty(1 << 28, dtype=torch.uint8, device="cuda"), torch.empty(1 << 28, dtype=torch.uint8, device="cuda"))
        self.timed(stream)                                   # (first launch: code object load, clocks)
        for _ in range(3):
            ms = self.timed(stream)
            if 0.8 * TARGET_MS <= ms <= 1.5 * TARGET_MS:
                break
            self.n = max(1, int(self.n * TARGET_MS / max(ms, 1e-3)))
        self.ms = self.timed(stream)
        if not 0.5 * TARGET_MS <= self.ms <= 4 * TARGET_MS:
            raise AssertionError("delay not calibrated: %s(%d) takes %.1f ms, wanted %.0f" % (self.kind, self.n, self.ms, TARGET_MS))

    def enqueue(self):
        """on the current stream"""
        if self._buf is None:
            self.torch.cuda._sleep(self.n)
        else:
            for _ in range(self.n):
                self._buf[1].copy_(self._buf[0], non_blocking=True)

    def timed(self, stream):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            e0.record()
            self.enqueue()
            e1.record()
        stream.synchronize()
        return e0.elapsed_time(e1)

    def __str__(self):
        return "%s(%d): %.1f ms" % (self.kind, self.n, self.ms)


class Late:
    """fills: [(dst, A, P)] device tensors of one size each (dst may be a slice of a padded buffer); outs: device tensors the call
    writes; call(stream): the entry point, stream = a raw handle or None (the context's own stream)."""

    def __init__(self, torch, ctx, stream, delay):
        assert stream.cuda_stream != 0
        self.torch, self.ctx, self.S, self.delay = torch, ctx, stream, delay
        self.host_ms = self.busy_at_return = None

    def _stage(self, fills, outs):
        for dst, _, p in fills:
            dst.copy_(p)
        for o in outs:
            sentinel(o)
        self.torch.cuda.synchronize()

    def warm(self, fills, outs, call):
        """the call once on P, drained: every workspace buffer of the context has its size, so that the late run allocates (and
        frees, which would drain the device and hide a misplaced step) nothing"""
        self._stage(fills, outs)
        call(None)
        self.ctx.sync()

    def run(self, fills, outs, call):
        """-> the outputs as they are on S right behind the call (host tensors).  host_ms: how long the call took on the host;
        busy_at_return: S had not finished when it returned (the whole call was queued inside the delay)."""
        torch, S = self.torch, self.S
        keep = [torch.empty_like(o) for o in outs]
        self._stage(fills, outs)
        with torch.cuda.stream(S):
            self.delay.enqueue()                             # S is busy for the delay
            for dst, a, _ in fills:
                dst.copy_(a, non_blocking=True)              # the real input arrives late
            t0 = time.perf_counter()
            call(S.cuda_stream)
            self.host_ms = (time.perf_counter() - t0) * 1e3
            self.busy_at_return = not S.query()
            for k, o in zip(keep, outs):
                k.copy_(o, non_blocking=True)                # consumed in stream order, no sync in between
        S.synchronize()
        return [k.cpu() for k in keep]

    def control(self, fills, outs, call):
        """the same set-up, the call on the context's own stream, unordered against S -> the outputs after everything has drained:
        expected(P) when the two streams run independently, expected(A) when they are serialised"""
        torch, S = self.torch, self.S
        self._stage(fills, outs)
        with torch.cuda.stream(S):
            self.delay.enqueue()
            for dst, a, _ in fills:
                dst.copy_(a, non_blocking=True)
        call(None)
        self.ctx.sync()                                      # (drains the device: S too)
        S.synchronize()
        return [o.cpu() for o in outs]
