"""Lane scheduling of ``map_images``: host threads, ordering and failure rules - no torch, no HIP (tests/test_lanes_host.py
drives it with stand-in lanes)."""
import itertools
import threading
from types import SimpleNamespace


class Turnstile:
    """Calls pass in index order, one at a time: ``wait(k)`` returns once 0 ... k - 1 are ``done``.  A call that fails does not
    say ``done``: ``abort`` makes every waiting and later ``wait`` raise, so nothing is issued out of sequence."""

    def __init__(self):
        self._cv = threading.Condition()
        self._next = 0
        self._error = None

    def wait(self, k, timeout=None):
        with self._cv:
            if not self._cv.wait_for(lambda: self._next == k or self._error is not None, timeout):
                raise TimeoutError(f"turn {k} did not come within {timeout} s (the turn is {self._next}'s)")
            if self._error is not None:
                raise RuntimeError("map_images: another lane failed before its gather") from self._error

    def done(self, k):
        with self._cv:
            if self._next == k:
                self._next = k + 1
            self._cv.notify_all()

    def abort(self, error):
        with self._cv:
            self._error = self._error or error
            self._cv.notify_all()


class Turnstiles(tuple):
    """One ``Turnstile`` per ordered stage of a call (``map_video(align=...)``: the denoise stage, then the align stage).  They fail
    together: a lane waiting at any stage must not wait for a call that will never reach it."""

    def abort(self, error):
        for t in self:
            t.abort(error)


def run_lanes(lanes, take, run, turnstile=None):
    """A generator over the outputs of ``run(lane_index, group, k)`` for every ``(k, group)`` that ``take()`` hands out (None: the
    input is exhausted; k counts from 0), in the order of k, as they complete.

    ``lanes``: one context manager per lane.  A lane is a host thread that enters its context (the pipeline's: a HIP stream) and
    then takes, runs and hands over one group after the other.  ONE lane runs inline in the caller's thread, with no thread
    at all.  ``take`` is never called by two lanes at once, and never more than ``len(lanes)`` groups ahead of the caller: a
    group counts as consumed when the caller comes back for the output after its last one, so ``take`` may draw from a lazy
    iterable.

    Failure: the first exception of ``take`` or ``run`` in any lane reaches the caller, after every output of a group with a lower
    k - those still running complete first.  It aborts ``turnstile`` (if given) before anything else happens, so lanes waiting
    for their turn raise and no turn is handed on past a failed one; no lane takes another group.  The generator returns, or is
    closed, with every thread joined."""
    if len(lanes) == 1:
        with lanes[0]:
            while (item := take()) is not None:
                yield from run(0, item[1], item[0])
        return
    cv, take_lock = threading.Condition(), threading.Lock()
    done = {}
    s = SimpleNamespace(taken=0, consumed=0, live=len(lanes), stop=False, failed=None)   # failed: (k, exception), the first one

    def work(i):
        k = float("inf")   # (a failure of take() is behind every group handed out)
        try:
            with lanes[i]:
                while True:
                    with cv:   # a slot of the look-ahead first; take() itself - it may load an image - runs outside cv
                        cv.wait_for(lambda: s.stop or s.taken - s.consumed < len(lanes))
                        if s.stop:
                            return
                        s.taken += 1
                    with take_lock:
                        item = take()
                    if item is None:
                        return
                    k = item[0]
                    out = run(i, item[1], k)
                    with cv:
                        done[k] = out
                        cv.notify_all()
                    k = float("inf")
        except BaseException as e:  # noqa: BLE001 - handed to the caller's thread
            if turnstile is not None:
                turnstile.abort(e)   # first: lanes waiting for their turn must not wait for a call that will never be made
            with cv:
                s.failed, s.stop = s.failed or (k, e), True
        finally:
            with cv:
                s.live -= 1
                cv.notify_all()

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(len(lanes))]
    for t in threads:
        t.start()
    try:
        for k in itertools.count():
            with cv:
                cv.wait_for(lambda: k in done or s.live == 0 or (s.failed and s.failed[0] <= k))
                if k not in done:   # a failure, or every lane has finished and group k was never started: the input is exhausted
                    break
                outs = done.pop(k)
            yield from outs
            with cv:
                s.consumed = k + 1
                cv.notify_all()
        if s.failed:
            raise s.failed[1]
    finally:
        with cv:
            s.stop = True
            cv.notify_all()
        for t in threads:
            t.join()
