"""A harness that runs the library on a non-default stream so that a stream mistake computes a wrong answer.

The suite's other GPU tests run with torch's current stream equal to the legacy null stream, which orders itself against
all other work: a kernel launched on the wrong stream, a copy or memset given the wrong stream, a wait on the wrong stream
and an output written under another stream than it was allocated for all give the right answer there.  Torch's pool
streams are non-blocking.  This module holds one of them (`side`), a calibrated delay, and two scenarios:

late_inputs   under `side`: the delay runs first, then every device input is produced on `side` (the real values copied
              over a poison pre-fill), then the library is called.  Whatever the library runs on another stream starts
              at once and reads poison; a wait on another stream returns host planes that still hold their poison.
busy_default  the delay is put on the null stream and the library runs under `side`.  Whatever the library queued on the
              null stream is held back behind the delay, and its consumers on `side` read stale intermediates.

Poison is finite, in range and wrong (a constant radiance inside the field's range, dmin in both range planes, zero
masks, zero depth planes, -1 in index planes): a library that did read it computes a wrong answer and cannot leave its
buffers.  No case is able to fault, even against a broken library.

The delay only has to outlast the host-side enqueue of one small call up to that call's first wait; nobody has measured
that time.  The controls in tests/test_gpu_side_stream.py hold the harness to its purpose whatever the number is: each
commits one of the mistakes on purpose and must see the wrong answer.

A plain module: importing it touches no device."""
from __future__ import annotations

import contextlib

import numpy as np

DELAY_TARGET_MS = 100.0
DELAY_MIN_MS = 50.0
SCENARIOS = ("late_inputs", "busy_default")

# poison (see above)
POISON_RADIANCE = 0.5        # normalised fields live in [0, 1]
POISON_LEVEL_U8 = 128.0      # raw uchar levels carried in float32
POISON_LEVEL_U16 = 32768.0   # raw ushort levels carried in float32
POISON_MASK = 0
POISON_DEPTH = 0.0
POISON_INDEX = -1


class Late:
    """A device input that exists late: `t` is pre-filled with poison before the scenario starts, the real values wait
    in `src`, and produce() copies them over the poison on the current stream (device to device: the host does not wait)."""

    def __init__(self, real: np.ndarray, poison):
        import torch
        real = np.ascontiguousarray(real)
        self.real = real
        self.src = torch.from_numpy(real.copy()).cuda()
        self.t = torch.full(tuple(real.shape), poison, dtype=self.src.dtype, device=self.src.device)
        assert real.size == 0 or not np.array_equal(self.t.cpu().numpy(), real), "the poison equals the real values"

    def produce(self):
        self.t.copy_(self.src, non_blocking=True)
        return self.t

    def reset(self, poison) -> None:
        self.t.fill_(poison)


class Scenario:
    def __init__(self, harness: "Harness", kind: str):
        assert kind in SCENARIOS, kind
        self.h, self.kind = harness, kind

    def arm(self) -> None:
        """Start the delay (again): on the side stream in late_inputs, on the null stream in busy_default.  Called on
        entry; a case whose first call waits calls it again before a later call it wants under test."""
        torch = self.h.torch
        if self.kind == "late_inputs":
            self.h.delay(self.h.side)
        else:
            self.h.delay(torch.cuda.default_stream(self.h.device))

    def produce(self, *lates: Late):
        """The device inputs, produced on the side stream (behind the delay in late_inputs)."""
        assert self.h.torch.cuda.current_stream(self.h.device) == self.h.side
        out = tuple(x.produce() for x in lates)
        return out[0] if len(out) == 1 else out


class Harness:
    """One non-blocking side stream and a calibrated delay on one device."""

    def __init__(self, device: int = 0):
        import torch
        assert torch.cuda.is_available(), "the stream harness needs a GPU"
        self.torch, self.device = torch, device
        torch.cuda.set_device(device)
        self.side = torch.cuda.Stream(device)
        assert self.side.cuda_stream != 0 and self.side != torch.cuda.default_stream(device)
        self.cycles = 1_000_000
        self.delay_ms = {}
        self._calibrate()

    def _measure(self, stream, cycles: int) -> float:
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            torch.cuda._sleep(int(cycles))
            b.record(stream)
        b.synchronize()
        return float(a.elapsed_time(b))

    def _calibrate(self) -> None:
        """The cycle count of a DELAY_TARGET_MS delay, measured with events on the streams the delay runs on; at least
        DELAY_MIN_MS on both or the module fails (it does not skip)."""
        torch = self.torch
        torch.cuda.synchronize(self.device)
        cycles, ms = self.cycles, 0.0
        for _ in range(5):
            ms = self._measure(self.side, cycles)
            if ms >= 5.0:
                break
            cycles *= 10
        assert ms >= 5.0, "torch.cuda._sleep(%d) took %.3f ms: no delay to calibrate" % (cycles, ms)
        self.cycles = int(cycles * DELAY_TARGET_MS / ms)
        for name, stream in (("side", self.side), ("null", torch.cuda.default_stream(self.device))):
            self.delay_ms[name] = self._measure(stream, self.cycles)
        assert min(self.delay_ms.values()) >= DELAY_MIN_MS, "the calibrated delay is too short: %r" % (self.delay_ms,)

    def delay(self, stream) -> None:
        with self.torch.cuda.stream(stream):
            self.torch.cuda._sleep(self.cycles)

    @contextlib.contextmanager
    def scenario(self, kind: str):
        """`with h.scenario(kind) as sc:` -- the body runs under the side stream with the delay armed; on exit both
        streams are drained, so results may be read on any stream afterwards."""
        torch = self.torch
        torch.cuda.synchronize(self.device)
        sc = Scenario(self, kind)
        try:
            with torch.cuda.stream(self.side):
                sc.arm()
                yield sc
        finally:
            torch.cuda.synchronize(self.device)

    @contextlib.contextmanager
    def on(self, stream):
        """The body runs under `stream` with nothing armed; drained on exit."""
        try:
            with self.torch.cuda.stream(stream):
                yield
        finally:
            self.torch.cuda.synchronize(self.device)


def host_poison(shape, dtype, value) -> np.ndarray:
    """A host output plane pre-filled with poison: a wait on the wrong stream hands it back as it is."""
    return np.full(shape, value, dtype=dtype)


def bits(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got: np.ndarray, want: np.ndarray, label) -> None:
    """Bit for bit (a NaN must be the same NaN)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    assert bad.size == 0, "%s: %d of %d values differ, first at %s: got %r want %r" % (
        label, bad.size, got.size, np.unravel_index(bad[0], got.shape), got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def assert_close(got: np.ndarray, want: np.ndarray, tol: float, label) -> None:
    """disp_confidence: the 1e-5 include/rslf_hip.h states (double arithmetic with a free summation order)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) if got.size else 0.0
    assert err <= tol, "%s: max |diff| %g > %g" % (label, err, tol)
