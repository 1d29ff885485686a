"""The stream gate of tests/test_gpu_stream_fidelity.py: a way to tell, from the bytes a call leaves, on which stream its device work ran.
No part of the package, no conftest and no pytest setting - a plain module.

A ``Call`` owns every device buffer of one call of one entry point: its inputs, its outputs, its workspace.  ``gated(stream, late)``
puts a bounded delay on a side stream and, behind it, ``late()``: only then do the input buffers receive the real inputs (until
then they hold a DECOY - the same scene reversed in memory order, a valid input with another answer) and only then are the outputs and
the workspace refilled with canaries.  The call is made with that stream's handle while the delay still runs.  Work that keeps to the
stream runs behind the gate and sees the real inputs; a launch or a memset that strays to another stream runs at once, on the decoy, and
what it writes is overwritten by the gate - or, where it reads what an earlier launch of the chain should have left, it reads canaries.
Either way the bytes differ from the call run alone.

The delay is ordinary device work of a fixed length (``torch.cuda._sleep``, or a chain of matrix products where that does not hold the
stream): nothing here waits for the host or for another stream, so a stream always drains by itself."""
import time

import numpy as np
import torch

PAD_BYTES = 64          # around every buffer; a multiple of 16, so the payload keeps the alignment of the allocation
CANARY, GARBAGE = 0xA5, 0x3C
MIN_DELAY_MS, HOST_FACTOR = 50.0, 20.0


class _Buffer:
    """``nbytes`` of device memory between two pads; everything is bytes on the device, the element type lives on the host"""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.whole = torch.full((self.nbytes + 2 * PAD_BYTES,), CANARY, dtype=torch.uint8, device="cuda")
        self.view = self.whole[PAD_BYTES:PAD_BYTES + self.nbytes]
        assert self.view.data_ptr() % 16 == 0

    def ptr(self):
        return self.view.data_ptr()

    @staticmethod
    def split(whole_host):
        """a host copy of ``whole`` -> its payload; the pads are checked on the way"""
        assert (whole_host[:PAD_BYTES] == CANARY).all() and (whole_host[-PAD_BYTES:] == CANARY).all(), "a pad was written"
        return whole_host[PAD_BYTES:-PAD_BYTES]


class Call:
    """The buffers of one call.  A row of the table builds one: ``inp`` / ``inout`` / ``out`` / ``ws`` / ``const`` return device addresses,
    ``launch(stream_handle) -> rc`` makes the call, ``check(result)`` (optional) holds the result to the restatement."""

    def __init__(self, name):
        self.name, self.inputs, self.outputs, self.scratch, self.alive = name, [], [], [], []
        self.launch = self.check = None

    @staticmethod
    def _bytes(array):
        return np.ascontiguousarray(array).reshape(-1).view(np.uint8)

    def inp(self, array, also_output=None):
        """an input: the device buffer, the real bytes and the decoy (the elements in reverse order), both uploaded beforehand"""
        if array is None:
            return None
        flat = np.ascontiguousarray(array).reshape(-1)
        buf = _Buffer(flat.nbytes)
        real = torch.from_numpy(self._bytes(flat).copy()).cuda()
        decoy = torch.from_numpy(self._bytes(flat[::-1]).copy()).cuda()
        self.inputs.append((buf, real, decoy, also_output))
        return buf.ptr()

    def inout(self, name, array):
        """an operand the call updates in place"""
        return self.inp(array, also_output=name)

    def out(self, name, dtype, count):
        buf = _Buffer(np.dtype(dtype).itemsize * int(count))
        self.outputs.append((name, np.dtype(dtype), buf))
        return buf.ptr()

    def ws(self, nbytes):
        buf = _Buffer(max(int(nbytes), 16))
        self.scratch.append(buf)
        return buf.ptr()

    def const(self, tensor_or_array):
        """device data that is no operand of the scene (weights, a colour table): uploaded once, never gated"""
        t = tensor_or_array if isinstance(tensor_or_array, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(tensor_or_array))
        t = t.cuda().contiguous()
        self.alive.append(t)
        return t.data_ptr()

    # -- what runs before the gate, behind it, and after the call; each on torch's current stream
    def arm(self):
        """the decoy into the inputs, garbage into everything the call writes"""
        for buf, _, decoy, _ in self.inputs:
            buf.view.copy_(decoy)
        for buf in [b for _, _, b in self.outputs] + self.scratch:
            buf.whole.fill_(GARBAGE)

    def late(self):
        """the real inputs, device to device, and the canaries"""
        for buf, real, _, _ in self.inputs:
            buf.view.copy_(real, non_blocking=True)
        for buf in [b for _, _, b in self.outputs] + self.scratch:
            buf.whole.fill_(CANARY)

    def snapshot(self):
        """device-to-device copies of everything the call may have touched"""
        return [b.whole.clone() for b, _, _, _ in self.inputs] + [b.whole.clone() for _, _, b in self.outputs] + [b.whole.clone() for b in self.scratch]

    def result(self, snapshot):
        """-> {output name: its bytes as a numpy array of the output's type}; pads intact, inputs untouched"""
        host = [t.cpu().numpy() for t in snapshot]
        got = {}
        for (buf, real, _, also_output), whole in zip(self.inputs, host):
            payload = _Buffer.split(whole)
            if also_output is None:
                assert np.array_equal(payload, real.cpu().numpy()), f"{self.name}: an input was written"
            else:
                got[also_output] = payload.copy()
        for (name, dtype, _), whole in zip(self.outputs, host[len(self.inputs):]):
            got[name] = _Buffer.split(whole).view(dtype).copy()
        for whole in host[len(self.inputs) + len(self.outputs):]:
            _Buffer.split(whole)
        return got


def same(a, b):
    """two results, byte for byte"""
    return a.keys() == b.keys() and all(a[k].tobytes() == b[k].tobytes() for k in a)


class Delay:
    """bounded device work of a known length on the current stream"""

    def __init__(self, kind, units, ms, slowest_host_ms):
        self.kind, self.units, self.ms, self.slowest_host_ms = kind, units, ms, slowest_host_ms
        self._m = torch.ones(1024, 1024, device="cuda") if kind == "matmul" else None

    def __call__(self):
        if self.kind == "sleep":
            torch.cuda._sleep(self.units)
        else:
            m = self._m
            for _ in range(self.units):
                m = (m @ self._m) * (1.0 / 1024)


def _measure(delay, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record()
        delay()
        b.record()
    stream.synchronize()
    return a.elapsed_time(b)


def calibrate(slowest_host_s, stream):
    """the delay whose measured time on the side stream ``stream`` is at least MIN_DELAY_MS and at least HOST_FACTOR times the slowest host call"""
    target = max(MIN_DELAY_MS, HOST_FACTOR * slowest_host_s * 1e3)
    for kind, first in (("sleep", 1_000_000), ("matmul", 16)):
        units, ms = first, 0.0
        for _ in range(24):   # (a bounded search: every trial is itself bounded device work)
            ms = _measure(Delay(kind, units, 0.0, 0.0), stream)
            if ms >= target:
                break
            units = int(units * max(2.0, min(64.0, 1.3 * target / max(ms, 1e-3))))
            if units > (10 ** 12 if kind == "sleep" else 10 ** 5):   # (this kind of work does not hold the stream here)
                break
        if ms >= target and _measure(Delay(kind, units, 0.0, 0.0), stream) >= target:
            return Delay(kind, units, ms, slowest_host_s * 1e3)
    raise AssertionError(f"no delay of {target:.0f} ms could be made on this device")


def gated(stream, late, delay):
    """the gate: on ``stream``, which does not wait for the null stream, the delay and then ``late()``"""
    with torch.cuda.stream(stream):
        delay()
        late()


def run_gated(calls, streams, delay):
    """every call of ``calls`` on its own stream behind its own gate, all made before any gate opens ->
    ([result], [whether the stream was still busy right after the call returned])"""
    for c in calls:
        c.arm()
    torch.cuda.synchronize()
    busy = []
    for c, s in zip(calls, streams):
        gated(s, c.late, delay)
        rc = c.launch(s.cuda_stream)
        busy.append(not s.query())
        assert rc == 0, (c.name, rc)
    busy = [b and not s.query() for b, s in zip(busy, streams)]   # (no gate had opened when the last call had been made)
    snaps = []
    for c, s in zip(calls, streams):
        with torch.cuda.stream(s):
            snaps.append(c.snapshot())
    for s in streams:
        s.synchronize()
    return [c.result(snap) for c, snap in zip(calls, snaps)], busy


def run_plain(call, stream):
    """the call alone, no gate: on ``stream``, or on the null stream with ``stream`` None -> (result, host seconds of the call)"""
    call.arm()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.default_stream()):
        call.late()
        t0 = time.perf_counter()
        rc = call.launch(None if stream is None else stream.cuda_stream)
        seconds = time.perf_counter() - t0
        assert rc == 0, (call.name, rc)
        snap = call.snapshot()
    torch.cuda.synchronize()
    return call.result(snap), seconds
