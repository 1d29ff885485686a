"""Host checks of ``map_images``' lane scheduling (marigold_amd/lanes.py) with stand-in lanes - ``contextlib.nullcontext()`` for the
stream, ``run`` callables that sleep a few milliseconds in a scrambled order - and of a stand-in pipeline whose lanes must see the
settings of the moment.  Every wait carries ``CAP`` seconds: a cap against deadlock (a deadlock fails the test), not a measurement."""
import contextlib
import threading
import time
from types import SimpleNamespace

import pytest
import torch

from marigold_amd.lanes import Turnstile, run_lanes
from marigold_amd.pipeline import MarigoldDepthPipeline
from marigold_amd.schedulers import DDIMScheduler, LCMScheduler

CAP = 20.0
SLEEP_MS = (9, 2, 6, 1, 8, 3, 5)   # per item: the later ones of a round of lanes finish first


def _capped(fn):
    """fn() in a thread of its own, joined with the cap -> its result; what it raised is raised here."""
    box = {}

    def target():
        try:
            box["result"] = fn()
        except BaseException as e:  # noqa: BLE001
            box["error"] = e
    t = threading.Thread(target=target, daemon=True)
    t.start()
    t.join(CAP)
    assert not t.is_alive(), f"deadlock: still running after {CAP} s"
    if "error" in box:
        raise box["error"]
    return box["result"]


def _source(n_items, n_lanes, received):
    """take() over n_items lazily produced items, checking that it is never entered twice at once and never runs more than
    n_lanes items ahead of what the consumer has received (``received``: a one-element list the consumer counts in)."""
    state = SimpleNamespace(pulled=0, inside=0, problems=[])
    guard = threading.Lock()

    def items():
        for k in range(n_items):
            state.pulled += 1
            if state.pulled - received[0] > n_lanes:
                state.problems.append(f"item {k} pulled with {received[0]} received: more than {n_lanes} ahead")
            yield k, [f"item{k}"]
    it = items()

    def take():
        with guard:
            state.inside += 1
            concurrent = state.inside > 1
        if concurrent:
            state.problems.append("take() entered by two lanes at once")
        time.sleep(0.001)
        try:
            return next(it, None)
        finally:
            with guard:
                state.inside -= 1
    return take, state


def _no_lane_threads_left(before):
    return [t for t in threading.enumerate() if t not in before and t is not threading.current_thread()] == []


@pytest.mark.parametrize("n_lanes", [1, 2, 3])
def test_outputs_in_input_order_take_serial_and_lazy(n_lanes):
    def scenario():
        before = set(threading.enumerate())
        received = [0]
        take, state = _source(7, n_lanes, received)
        lanes_used = set()

        def run(lane, group, k):
            lanes_used.add(lane)
            time.sleep(SLEEP_MS[k] / 1000.0)
            return [(k, group[0])]
        got = []
        for out in run_lanes([contextlib.nullcontext() for _ in range(n_lanes)], take, run):
            got.append(out)
            received[0] += 1
        assert got == [(k, f"item{k}") for k in range(7)]
        assert state.problems == [] and state.pulled == 7
        assert lanes_used <= set(range(n_lanes)) and (n_lanes == 1 or len(lanes_used) > 1)
        assert _no_lane_threads_left(before)
    _capped(scenario)


def test_lazy_input_is_not_drained_behind_a_slow_consumer():
    """Three lanes, a consumer that takes its time: the lanes wait instead of pulling the whole input."""
    def scenario():
        received = [0]
        take, state = _source(7, 3, received)
        gen = run_lanes([contextlib.nullcontext() for _ in range(3)], take, lambda lane, group, k: [k])
        assert next(gen) == 0
        received[0] += 1
        time.sleep(0.05)   # every lane is long done with what it may take
        assert state.pulled <= 1 + 3
        rest = []
        for out in gen:
            rest.append(out)
            received[0] += 1
        assert rest == list(range(1, 7)) and state.problems == []
    _capped(scenario)


def test_turnstile_orders_the_gathers_whichever_lane_finishes_first():
    def scenario():
        ts, record = Turnstile(), []
        received = [0]
        take, state = _source(7, 3, received)

        def run(lane, group, k):
            time.sleep(SLEEP_MS[k] / 1000.0)   # the prediction: map 1 is ready long before map 0
            ts.wait(k, timeout=CAP)
            record.append(k)                   # the "gather"
            ts.done(k)
            return [k]
        got = []
        for out in run_lanes([contextlib.nullcontext() for _ in range(3)], take, run, ts):
            got.append(out)
            received[0] += 1
        assert record == list(range(7)) and got == list(range(7)) and state.problems == []
    _capped(scenario)


def test_failed_gather_aborts_the_turnstile_before_the_turn_moves():
    """Map 2's gather raises: no later gather is issued, the lanes waiting for their turn raise, the caller gets maps 0 and 1 and
    then map 2's error."""
    def scenario():
        before = set(threading.enumerate())
        ts, record, refused = Turnstile(), [], []
        take, _ = _source(7, 3, [7])

        def run(lane, group, k):
            time.sleep(SLEEP_MS[k] / 1000.0)
            try:
                ts.wait(k, timeout=CAP)
            except RuntimeError:
                refused.append(k)
                raise
            if k == 2:
                time.sleep(0.02)   # maps 3 and 4 are at the turnstile by now
                raise OSError("gather 2 failed")
            record.append(k)
            ts.done(k)
            return [k]
        got = []
        with pytest.raises(OSError, match="gather 2 failed"):
            for out in run_lanes([contextlib.nullcontext() for _ in range(3)], take, run, ts):
                got.append(out)
        assert got == [0, 1]
        assert record == [0, 1]
        assert refused and all(k > 2 for k in refused)   # they raised; the cap never ran out (that would be a TimeoutError)
        with pytest.raises(RuntimeError, match="another lane failed"):
            ts.wait(3, timeout=CAP)
        assert _no_lane_threads_left(before)
    _capped(scenario)


def test_error_without_a_turnstile_comes_after_the_finished_maps():
    """Map 3 fails while maps 0 to 2 have finished or are still running: the caller gets 0, 1, 2, then the exception, and the
    function returns with every thread joined."""
    def scenario():
        before = set(threading.enumerate())
        take, state = _source(7, 3, [7])

        def run(lane, group, k):
            if k == 3:
                raise KeyError("map 3")
            time.sleep((30 if k == 2 else SLEEP_MS[k]) / 1000.0)   # map 2 is still running when map 3 fails
            return [k]
        got = []
        with pytest.raises(KeyError, match="map 3"):
            for out in run_lanes([contextlib.nullcontext() for _ in range(3)], take, run):
                got.append(out)
        assert got == [0, 1, 2]
        assert state.pulled <= 3 + 3   # no lane went on taking
        assert _no_lane_threads_left(before)
    _capped(scenario)


def test_error_in_take_and_a_closed_generator_leave_no_thread():
    def scenario():
        before = set(threading.enumerate())
        calls = [0]

        def take():
            calls[0] += 1
            if calls[0] == 4:
                raise ValueError("bad input 3")
            return calls[0] - 1, [calls[0] - 1]
        got = []
        with pytest.raises(ValueError, match="bad input 3"):
            for out in run_lanes([contextlib.nullcontext() for _ in range(2)], take, lambda lane, group, k: [k]):
                got.append(out)
        assert got == [0, 1, 2]
        take2, _ = _source(7, 3, [7])
        gen = run_lanes([contextlib.nullcontext() for _ in range(3)], take2, lambda lane, group, k: [k])
        assert next(gen) == 0
        gen.close()   # the caller walks away
        assert _no_lane_threads_left(before)
    _capped(scenario)


# ---- a stand-in pipeline: the lanes of every call see the settings of its moment ------------------------------------------------

class _SettingsStandIn(MarigoldDepthPipeline):
    """Engines are namespaces that count their replicas; a call returns the settings it sees; three lanes run on the host."""

    def __init__(self):
        self.replicas = []

        def engine(name):
            def replica():
                self.replicas.append(name)
                return SimpleNamespace(name=f"{name} replica {len(self.replicas)}", device=device)
            return SimpleNamespace(name=name, device=device, replica=replica)
        device = SimpleNamespace(type="cuda")   # (what map_images asks before it runs more than one lane)
        super().__init__(engine("unet"), engine("vae"), DDIMScheduler(), default_denoising_steps=4, default_processing_resolution=0,
                         empty_text_embed=torch.zeros(1, 2, 4))
        self.force_sharded = False

    def _sharded(self):
        return self.force_sharded or super()._sharded()

    def _lane_stream(self):
        return None

    def _lane_contexts(self, streams):
        return [contextlib.nullcontext() for _ in streams], lambda: None

    def __call__(self, image, **kw):
        time.sleep(SLEEP_MS[image % 7] / 1000.0)
        turn = self._gather_turn
        if self._sharded():   # the gather of a member-parallel pipeline, in its turn
            turn[0].wait(turn[1], timeout=CAP)
            turn[0].done(turn[1])
        return (self.default_denoising_steps, type(self.scheduler).__name__, self._sharded(), self.unet.name, turn is not None)


def test_lanes_see_settings_changed_between_calls():
    def scenario():
        pipe = _SettingsStandIn()
        first = list(pipe.map_images(range(7), in_flight=3))
        assert [o[:3] for o in first] == [(4, "DDIMScheduler", False)] * 7 and not any(o[4] for o in first)
        assert len({o[3] for o in first}) == 3   # three lanes ran, each over engines of its own
        lanes = list(pipe._lanes)
        assert len(lanes) == 3 and lanes[0][0].unet is pipe.unet and lanes[0][0].vae is pipe.vae and sorted(pipe.replicas) == ["unet"] * 2 + ["vae"] * 2
        scheduler = LCMScheduler()
        pipe.scheduler = scheduler
        pipe.default_denoising_steps = 1
        pipe.enable_member_parallel()
        pipe.force_sharded = True
        second = list(pipe.map_images(range(7), in_flight=3))
        assert [o[:3] for o in second] == [(1, "LCMScheduler", True)] * 7 and all(o[4] for o in second)
        assert "_gather_turn" not in vars(pipe) and pipe._gather_turn is None
        assert pipe.scheduler is scheduler   # the lanes worked on copies
        assert len(pipe._lanes) == 3 and all(a is b for x, y in zip(lanes, pipe._lanes) for a, b in zip(x, y))
        assert pipe.replicas.count("unet") == 2 and pipe.replicas.count("vae") == 2   # replica() twice per engine in total, not four times
    _capped(scenario)
