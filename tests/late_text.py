"""A text that arrives late on the caller's stream: every entry that reads device text must read it IN STREAM ORDER.  Behind
tests/test_gpu_caller_stream.py, checked on the CPU by tests/test_late_text_host.py.

A scan context made on a caller's stream (seeqdevScanNew(hip_stream), Scanner(stream)) promises that its launches, copies and memsets are
ordered behind everything queued on that stream at the time of the call.  Everywhere else in the suite the context's stream is of the default,
"blocking" kind and the text's producer ran on the legacy null stream, so the null stream's implicit barrier orders the two whatever the
context does.  A PyTorch caller on a side stream passes a NON-BLOCKING stream, which has no such barrier.  Here the text's producer is made
visibly late on such a stream:

  decoy(window)   the window with C G T c g t mapped to A / a and every other byte kept: a valid text of the same lines and records with other
                  answers.  A kernel that reads it never leaves the window and parses the same records.
  LateText        device copies of the true bytes and of the decoy.  arm() enqueues on the side stream, and does nothing else:
                  copy decoy -> t, a device-side delay (torch.cuda._sleep: one thread that spins, no host sleep, no kernel that fills the
                  machine), copy true -> t.  It never waits on the host.
  LateScanner     a Scanner on the side stream that arms before every method that reads device text, and asserts right before the entry
                  gets control that the producer is still pending (`not side.query()`): a condition, not a measurement -- an arm that was
                  not pending proved nothing and fails the test.  It does not arm again between run and fetch: a fall-back re-run reads the
                  text again, and the caller keeps the text until the fetch.
  LatePacked      the same for run_packed, whose input is not the text but what was packed from it: the packed arrays are cleared, the text
                  is armed and the packing queued behind it, so the arrays are zeros until the delay is over.

An entry that is ordered answers over the true bytes.  One that launched, copied or uploaded off the stream, or did not wait for an upload,
reads the decoy (or a table that is not there yet) and answers something else: tests/test_late_text_host.py shows, with the references
alone, that the decoy's answers differ in every quantity the GPU module compares.

A plain helper module: no fixtures, no test collection."""
import ctypes
import inspect
import time

from seeq_amd import device as dev

_DECOY = bytes.maketrans(b"CGTcgt", b"AAAaaa")
MIN_DELAY_MS = 5.0
HIP_STREAM_NON_BLOCKING = 1

# the methods of dev.Scanner that read device text (a parameter of one of these names), each armed by LateScanner
TEXT_PARAMS = ("t", "d_ptr", "bases_ptr")
ARMED = ("run", "scan_tensor", "strands_tensor", "inserts_tensor", "insert_text", "scan_tensor_multi", "demux_tensor", "tally", "tally_hold",
         "tally_grouped", "tally_library", "tally_hold_library", "quality_gate", "run_packed")
# public methods with such a parameter that are NOT armed: name -> why
EXEMPT = {}


def decoy(window):
    return bytes(window).translate(_DECOY)


def text_methods():
    """{name: parameter} of dev.Scanner's public methods that take device text"""
    out = {}
    for name, fn in inspect.getmembers(dev.Scanner, callable):
        if name.startswith("_"):
            continue
        fn = inspect.unwrap(fn)
        params = inspect.signature(fn).parameters
        hit = [p for p in TEXT_PARAMS if p in params]
        if hit:
            out[name] = hit[0]
    return out


def stream_flags(stream):
    """hipStreamGetFlags of a torch stream through the HIP runtime the process has loaded; None where it cannot be reached"""
    try:
        fn = ctypes.CDLL(None).hipStreamGetFlags
    except (OSError, AttributeError):
        return None
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint)]
    flags = ctypes.c_uint(0)
    return int(flags.value) if fn(ctypes.c_void_p(stream.cuda_stream), ctypes.byref(flags)) == 0 else None


class Delay:
    """torch.cuda._sleep calibrated once with two events: `cycles_per_ms`.  cycles(ms) -> the argument for a delay of ms."""

    def __init__(self):
        import torch
        s = torch.cuda.Stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            torch.cuda._sleep(1000)                             # (the kernel's first launch loads it)
            s.synchronize()
            cycles, ms = 1000000, 0.0
            for _ in range(3):                                  # (a span of at least 2 ms, so that the launch is small beside it)
                e0.record(s)
                torch.cuda._sleep(cycles)
                e1.record(s)
                e1.synchronize()
                ms = e0.elapsed_time(e1)
                if ms >= 2.0:
                    break
                cycles = int(cycles * 10.0 / max(ms, 0.001))
        assert ms >= 2.0, "torch.cuda._sleep(%d) took %.3f ms: the delay cannot be calibrated" % (cycles, ms)
        self.cycles_per_ms = cycles / ms

    def cycles(self, ms):
        return max(1, int(ms * self.cycles_per_ms))


class LateText:
    """t: the view's CUDA tensor (uint8, the window's bytes); side: a torch.cuda.Stream()."""

    def __init__(self, t, window, side):
        import torch
        assert t.is_cuda and t.dtype == torch.uint8 and t.numel() == len(window)
        self.t, self.window, self.side = t, bytes(window), side
        self.true = torch.frombuffer(bytearray(self.window), dtype=torch.uint8).cuda()
        self.decoy = torch.frombuffer(bytearray(decoy(self.window)), dtype=torch.uint8).cuda()
        self.arms = 0
        torch.cuda.synchronize()

    def arm(self, cycles):
        """decoy -> t, the delay, true -> t, on the side stream; no host wait."""
        import torch
        with torch.cuda.stream(self.side):
            self.t.copy_(self.decoy, non_blocking=True)
            torch.cuda._sleep(cycles)
            self.t.copy_(self.true, non_blocking=True)
        self.arms += 1

    def put_decoy(self):
        """The decoy in place, waited for on the host -- not part of an arm: for the liveness proof alone, whose context is ordered behind
        NOTHING on the side stream and must still find the decoy whenever it looks (the arm that follows copies the same bytes again)."""
        import torch
        with torch.cuda.stream(self.side):
            self.t.copy_(self.decoy, non_blocking=True)
        self.side.synchronize()

    def pending(self):
        assert not self.side.query(), "arm %d: the side stream has run dry before the entry got control: the arm proves nothing" % self.arms


class LatePacked:
    """Packed reads that arrive late: `bases` / `nmask` (CUDA uint8 tensors) are what pack() -- a callable that enqueues the packing of
    text.t on the side stream -- fills.  arm() enqueues on the side stream: clear both arrays, the text's own arm (decoy, delay, true
    bytes), the packing.  Until the delay is over the arrays hold zeros -- reads of A alone, a valid batch with other answers."""

    def __init__(self, text, bases, nmask, pack):
        self.text, self.bases, self.nmask, self.pack = text, bases, nmask, pack

    def clear(self):
        import torch
        with torch.cuda.stream(self.text.side):
            self.bases.zero_()
            self.nmask.zero_()

    def arm(self, cycles):
        self.clear()
        self.text.arm(cycles)
        self.pack()

    def put_zeros(self):
        """the cleared arrays in place, waited for on the host: for the liveness proof alone (LateText.put_decoy)"""
        self.clear()
        self.text.side.synchronize()


class LateScanner(dev.Scanner):
    """A Scanner on side.cuda_stream.  give(t, window) names a text; every ARMED method called with that tensor (or its address) arms it
    first; run_packed arms the batch named by give_packed (LatePacked: its arrays cleared, its text armed and packed again, all on the
    stream); a method called with t=None (the text a host entry staged) gets a bare delay in front of it.  armed=False: nothing is
    queued, and `slowest_ms` is the wall time of the slowest call -- what the delay is sized from.  `arms`: how often a producer was
    pending when an entry got control."""

    def __init__(self, side, cycles=0, armed=True):
        assert side.cuda_stream, "the side stream is the null stream"
        super().__init__(side.cuda_stream)
        self.side, self.cycles, self.armed = side, cycles, armed
        self.texts, self.packed, self.depth, self.arms, self.slowest_ms = {}, None, 0, 0, 0.0

    def give(self, t, window):
        key = (t.data_ptr(), t.numel())
        if key not in self.texts:
            self.texts[key] = LateText(t, window, self.side)
        return self.texts[key]

    def give_packed(self, t, window, bases, nmask, pack):
        self.packed = LatePacked(self.give(t, window), bases, nmask, pack)
        return self.packed

    def bare(self):
        """a bare delay pending on the side stream"""
        import torch
        with torch.cuda.stream(self.side):
            torch.cuda._sleep(self.cycles)
        assert not self.side.query(), "the bare delay has run out before the entry got control"
        self.arms += 1

    def arm(self, text):
        """text: a tensor, a device address, or None"""
        if text is None:
            return self.bare()
        ptr = text if isinstance(text, int) else text.data_ptr()
        late = next((lt for (p, n), lt in self.texts.items() if p == ptr), None)
        assert late is not None, "a text this LateScanner has not been given: %#x" % ptr
        late.arm(self.cycles)
        late.pending()
        self.arms += 1

    def arm_packed(self, bases_ptr):
        assert self.packed is not None and self.packed.bases.data_ptr() == bases_ptr, "a packed batch this LateScanner has not been given"
        self.packed.arm(self.cycles)
        self.packed.text.pending()
        self.arms += 1

    def _late(self, arm, call):
        if self.depth:                                          # (scan_tensor calls run: one arm per call from outside)
            return call()
        self.depth += 1
        try:
            if self.armed:
                arm()
                return call()
            t0 = time.perf_counter()
            res = call()
            self.slowest_ms = max(self.slowest_ms, (time.perf_counter() - t0) * 1e3)
            return res
        finally:
            self.depth -= 1


def _armed_method(name):
    base = getattr(dev.Scanner, name)
    sig = inspect.signature(base)
    param = next(p for p in TEXT_PARAMS if p in sig.parameters)

    def method(self, *args, **kw):
        bound = sig.bind(self, *args, **kw)
        bound.apply_defaults()
        text = bound.arguments[param]
        arm = (lambda: self.arm_packed(text)) if param == "bases_ptr" else (lambda: self.arm(text))
        return self._late(arm, lambda: base(self, *args, **kw))
    method.__name__, method.__doc__ = name, base.__doc__
    return method


for _name in ARMED:
    setattr(LateScanner, _name, _armed_method(_name))
