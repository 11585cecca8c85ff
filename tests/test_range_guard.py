"""The fp16 range guard's word protocol, host side (no GPU): a fake stands in for the library the guard loads, and
where a case reaches a stream synchronize ``torch.cuda.current_stream`` is replaced."""
import os
import sys
import threading
import time

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from renderformer_amd import range_guard  # noqa: E402


class FakeLib:
    """rf_range_word_*: integer handles, a log of (call, handle) in call order, settable codes."""

    def __init__(self):
        self.log, self.codes, self.live, self.freed = [], {}, set(), []
        self._next = 100
        self._lock = threading.Lock()

    def rf_range_word_new(self, ref):
        with self._lock:
            self._next += 1
            h = self._next
            self.live.add(h)
            self.log.append(("new", h))
        ref._obj.value = h
        return 0

    def rf_range_word_clear(self, h):
        self.codes[h] = 0
        self.log.append(("clear", h))
        return 0

    def rf_range_word_bind(self, h):
        self.log.append(("bind", h))
        return 0

    def rf_range_word_read(self, h):
        self.log.append(("read", h))
        return self.codes.get(h, 0)

    def rf_range_word_free(self, h):
        self.log.append(("free", h))
        self.live.discard(h)
        self.freed.append(h)
        return 0

    def rf_last_error(self):
        return b""

    def calls(self, name):
        return [h for n, h in self.log if n == name]


class Model:  # what the guard reads of a RenderFormer (none of it in these cases)
    range_check, operands, dpt_precision = "sync", "f16", "f16"


@pytest.fixture
def guard(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(range_guard, "_load_lib", lambda: lib)
    model = Model()
    g = range_guard.RangeGuard(model)
    g.test_model, g.lib = model, lib  # (the guard holds its model weakly)
    return g


def test_bound_reuses_the_pooled_word_and_close_frees_every_word_once(guard):
    """A word stays out of the pool from bound() until take() has read it (its frame may still write it)."""
    lib = guard.lib
    with guard.bound() as a:
        assert lib.log[-1] == ("bind", a)
    assert not guard.free and guard.take(a) == (0, []) and guard.free == [a]
    with guard.bound() as b:
        assert not guard.free
    assert a == b and lib.calls("new") == [a]
    assert lib.log == [("new", a), ("clear", a), ("bind", a), ("bind", None), ("read", a),
                       ("clear", a), ("bind", a), ("bind", None)]
    with guard.bound() as c:  # the first word is still unread: the pool is empty, a second one is made
        assert c != a
    guard.take(a)
    guard.close()  # (c was never read: it is its holder's, like a pending frame's, and close() frees the pooled ones)
    assert lib.freed == [a]
    guard.take(c)
    guard.close()
    assert sorted(lib.freed) == sorted(lib.calls("new")) == sorted([a, c]) and not lib.live
    assert not guard.free and not guard.pending


class _Stream:
    def __init__(self, guard, fail):
        self.guard, self.fail, self.seen = guard, fail, None

    def synchronize(self):
        # (what had happened when the wait began: the unbind logged, the word not yet back in the pool)
        self.seen = (self.guard.lib.log[-1], list(self.guard.free))
        if self.fail:
            raise RuntimeError("synchronize after a device-side error")


@pytest.mark.parametrize("sync_fails", [True, False])
def test_a_raising_body_unbinds_waits_and_returns_the_word(guard, monkeypatch, sync_fails):
    """The body's own exception propagates even when the stream wait raises too, and the word goes back to the
    pool either way; the order is unbind, wait, return."""
    stream = _Stream(guard, sync_fails)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: stream)
    with pytest.raises(ValueError, match="boom"):
        with guard.bound() as word:
            raise ValueError("boom")
    assert guard.lib.calls("bind")[-1] is None
    assert stream.seen == (("bind", None), [])
    assert guard.free == [word]


@pytest.mark.parametrize("code, names", [(0, []), (1, ["GEMM"]), (8, ["DPT plane"]),
                                         (13, ["GEMM", "attention", "DPT plane"])])
def test_take_names_the_writers_and_returns_the_word(guard, code, names):
    with guard.bound() as word:
        guard.lib.codes[word] = code  # (raised by a kernel while the word was bound)
    assert not guard.free
    assert guard.take(word) == (code, names)
    assert guard.free == [word] and guard.lib.log[-1] == ("read", word)


def test_threads_never_share_a_word(guard):
    held, clash, lock = set(), [], threading.Lock()
    start = threading.Barrier(2)

    def work():
        start.wait()
        for _ in range(50):
            with guard.bound() as word:
                with lock:
                    if word in held:
                        clash.append(word)
                    held.add(word)
                time.sleep(0)  # (yield: let the other thread take its word while this one is held)
                with lock:
                    held.discard(word)
            guard.take(word)

    threads = [threading.Thread(target=work) for _ in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not clash
    assert 1 <= len(guard.lib.calls("new")) <= 2
    assert sorted(guard.free) == sorted(guard.lib.calls("new"))
