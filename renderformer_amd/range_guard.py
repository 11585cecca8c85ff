"""The fp16 range check of a RenderFormer (its modes: RenderFormer.__init__): the pool of host-mapped range words
that the fp16-writing kernels raise on |x| > 65504, the frames whose word is not yet read, and the re-render after a
fallback.  The model's ``range_check``, ``operands`` and ``dpt_precision`` are read live at every call; moving the
model to other operands stays its own ``_fall_back``."""
import contextlib
import ctypes
import threading
import weakref
from typing import List, Optional

import torch

from ._lib import DeviceError
from ._lib import load as _load_lib

RANGE_WORDS_MAX = 8  # frames with an unresolved range word per model; the oldest is resolved (waited for) beyond
RANGE_CODES = (("GEMM", 1), ("RMSNorm", 2), ("attention", 4), ("DPT plane", 8))  # fp16 writer -> bit of the word


def deferred_error(code: int, names, remedy: str, where: str = "") -> DeviceError:
    """The "deferred" mode's report of an overflowed frame (or, with ``where``, scene encode)."""
    return DeviceError(f"fp16 operand overflow (range code {code}: |x| > 65504 in an fp16 {'/'.join(names)} "
                       f"output){where} -- this checkpoint's activations exceed fp16's range: {remedy}")


class _Frame:
    """A rendered frame whose fp16 range word is not yet read: the word, the frame's end event and stream, the
    output tensor, a replay closure (the same render with the texture already log-encoded) and the inputs'
    version counters (an input edited in place since the render cannot be replayed)."""
    __slots__ = ("word", "event", "stream", "out", "replay", "inputs", "versions")

    def __init__(self, word, event, stream, out, replay, inputs):
        self.word, self.event, self.stream, self.out, self.replay = word, event, stream, out, replay
        self.inputs = inputs
        self.versions = [t._version for t in inputs]


class RangeGuard:
    """The range words and pending frames of one model.  The lock guards the two lists only: the binding itself is
    per thread (rf_range_word_bind).  The library is loaded on first use: constructing a model touches no device."""

    def __init__(self, model):
        self.model = weakref.proxy(model)  # (the model owns the guard: no cycle, it is released by its last reference)
        self.free: List[int] = []  # range-word handles not in use
        self.pending: List[_Frame] = []  # frames whose word is unread, oldest first
        self.lock = threading.RLock()

    def active(self) -> bool:
        m = self.model
        return (m.operands == "f16" or m.dpt_precision == "f16") and m.range_check != "off"

    def _release(self, word):
        with self.lock:
            self.free.append(word)

    @contextlib.contextmanager
    def bound(self):
        """A word of the pool (a new one when it is empty), cleared and bound to this thread while the body runs."""
        lib = _load_lib()
        with self.lock:
            word = self.free.pop() if self.free else None
        if word is None:
            h = ctypes.c_void_p()
            if lib.rf_range_word_new(ctypes.byref(h)) != 0:
                raise RuntimeError(f"rf_range_word_new: {lib.rf_last_error().decode(errors='replace')}")
            word = h.value
        lib.rf_range_word_clear(word)
        lib.rf_range_word_bind(word)
        try:
            yield word
        except BaseException:
            # a refused launch (validation / DeviceError): whatever did run reads the word only on this stream
            lib.rf_range_word_bind(None)
            try:
                torch.cuda.current_stream().synchronize()
            except Exception:  # after a device-side error the wait can raise too: the body's error is the report
                pass
            finally:
                self._release(word)
            raise
        lib.rf_range_word_bind(None)

    def take(self, word):
        """Read a word whose launches have completed and return it to the pool: (code, names of the writers)."""
        code = int(_load_lib().rf_range_word_read(word))
        self._release(word)
        return code, [n for n, bit in RANGE_CODES if code & bit]

    def run(self, run, replay, inputs):
        """Run one render under a range word of its own; resolve it now (sync) or later (lazy / deferred)."""
        if not self.active():
            return run()
        self._poll()
        with self.bound() as word:
            out = run()
        stream = torch.cuda.current_stream()
        ev = torch.cuda.Event()
        ev.record(stream)
        fr = _Frame(word, ev, stream, out, replay, inputs)
        if self.model.range_check == "sync":
            self._resolve(fr, wait=True)
            return out
        with self.lock:
            self.pending.append(fr)
            oldest = self.pending.pop(0) if len(self.pending) > RANGE_WORDS_MAX else None
        if oldest is not None:
            self._resolve(oldest, wait=True)
        return out

    def _poll(self):
        """Resolve (oldest first) the pending frames whose end event has completed: no host wait."""
        while True:
            with self.lock:
                if not (self.pending and self.pending[0].event.query()):
                    return
                fr = self.pending.pop(0)
            self._resolve(fr, wait=False)

    def _resolve(self, fr: _Frame, wait: bool, stacklevel: int = 5) -> bool:
        """Read a frame's word (after its end event); on an overflow fall back and re-render it in place (lazy /
        sync) or raise DeviceError (deferred).  Returns True if the frame was rendered again.  The caller has taken
        ``fr`` off the pending list, so no other thread resolves it.  ``stacklevel``: the fallback warning's."""
        if wait:
            fr.event.synchronize()
        code, what = self.take(fr.word)
        if not code:
            return False
        m = self.model
        if m.range_check == "deferred":
            raise deferred_error(code, what, "render with operands='bf16' (RF_OPERANDS=bf16) and "
                                 "dpt_precision='bf16x3', or range_check='sync' / 'lazy' (re-renders such frames)")
        if any(t._version != v for t, v in zip(fr.inputs, fr.versions)):
            raise DeviceError(f"fp16 operand overflow (range code {code}) in a frame whose inputs were modified in "
                              "place before it could be rendered again: call resolve(out) / check_range() before "
                              "reusing input buffers, or use range_check='sync'")
        m._fall_back(code, what, "frame is rendered again", stacklevel=stacklevel)
        with torch.cuda.device(m._device), torch.cuda.stream(fr.stream):
            new = self.replay(fr.replay)
            fr.out.copy_(new.view_as(fr.out))
        fr.out._rf_rerendered = True  # resolve(out) reports it even when a later render's poll did the re-render
        return True

    def replay(self, replay):
        """The re-render after a fallback, checked at once: an overflow that survives it is an error."""
        if not self.active():
            return replay()
        with self.bound() as word:
            out = replay()
        torch.cuda.current_stream().synchronize()
        code, _ = self.take(word)
        if code:
            raise DeviceError(f"fp16 overflow (range code {code}) persists after the bf16 fallback")
        return out

    def resolve(self, out: Optional[torch.Tensor] = None) -> bool:
        """RenderFormer.resolve: the frame whose output is ``out`` (every pending frame if None), waiting for it."""
        with self.lock:
            keep, done = [], []
            for fr in self.pending:
                (done if out is None or fr.out is out else keep).append(fr)
            self.pending = keep
        for fr in done:
            self._resolve(fr, wait=True, stacklevel=6)  # (one frame deeper than a render: the model's delegation)
        redo = False
        for t in ([fr.out for fr in done] if out is None else [out]):
            if getattr(t, "_rf_rerendered", False):
                t._rf_rerendered = False
                redo = True
        return redo

    def check_range(self):
        """RenderFormer.check_range: resolve every pending frame, waiting for each."""
        with self.lock:
            pending, self.pending = self.pending, []
        for i, fr in enumerate(pending):
            try:
                self._resolve(fr, wait=True, stacklevel=6)
            except BaseException:
                for rest in pending[i + 1:]:  # the others' words stay usable
                    rest.event.synchronize()
                    self._release(rest.word)
                raise

    def close(self):
        """RenderFormer.close: free every range word, waiting for the pending frames first."""
        with self.lock:
            words = list(self.free)
            for fr in self.pending:
                fr.event.synchronize()
                words.append(fr.word)
            self.free, self.pending = [], []
        for w in words:
            _load_lib().rf_range_word_free(w)
