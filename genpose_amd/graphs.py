"""The host layer's two small protocols, written once: capture a launch sequence once per shape, then replay it (`capture`,
`Captured.replay`, `release`, `CapturedPasses`), and upload a small host block in stream order through one pinned buffer (`PinnedBlock`;
`UploadRing`: a rotation of such blocks, for an owner that uploads on every call and must not wait for the call before).

A pin is a count on a workspace dict (`_pins`): a workspace with a count above zero stays out of its cache's eviction order
(`unpinned`).  Its buffers were allocated outside the capture and nothing but that cache holds them, so it must outlive every graph that
writes into it.  `pin` and `unpin` are the only writers of the count.
"""
import contextlib
import gc

import torch

from .lru import ShapeCache


def pin(ws):
    ws["_pins"] = ws.get("_pins", 0) + 1
    return ws


def unpin(ws):
    ws["_pins"] -= 1


def unpinned(ws):  # (can_evict of a workspace cache)
    return ws.get("_pins", 0) == 0


@contextlib.contextmanager
def holding(pins):
    """pins: callables that each take one pin and return its workspace (Pointnet2EncoderHIP.pin_workspaces, `pin` on a dict).  Yields the
    pinned workspaces, which stay pinned when the block ends - they go into the `Captured` entry, whose `release` gives them back - and
    are given back here if the block (or a later pin) raises: a failed capture leaves every count where it was."""
    pinned = []
    try:
        pinned.extend(take() for take in pins)  # (one by one: the pins taken before one that raises are in the list)
        yield pinned
    except BaseException:
        for ws in pinned:
            unpin(ws)
        raise


class Captured:
    """One entry of a cache of captured graphs: the graph, its static inputs `bufs`, its static outputs `outs` (whatever the captured body
    returned; the next replay overwrites them), the workspaces whose pins it holds, and what else the site keeps with it (`extra`)."""

    def __init__(self, graph, bufs, outs, pinned, extra):
        self.graph, self.bufs, self.outs, self.pinned, self.extra = graph, bufs, outs, pinned, extra

    def replay(self, *inputs, events=None):
        """Copies `inputs` into the static buffers and replays, between `events`' two events where given; returns the static outputs."""
        for b, v in zip(self.bufs, inputs):
            b.copy_(v)
        if events is not None:
            events[0].record(torch.cuda.current_stream())
        self.graph.replay()
        if events is not None:
            events[1].record(torch.cuda.current_stream())
        return self.outs


def release(key, ent):
    """The on_evict of every cache of `Captured` entries (a plain function, no closure over the cache's owner: no reference cycle): the
    workspaces the entry's replays wrote into return to the eviction order."""
    for ws in ent.pinned:
        unpin(ws)


def capture(body, bufs=(), pins=(), stream=None, warmup=None, extra=None):
    """Captures the launches `body()` issues (on `stream`, else the current one) and returns the `Captured` entry; body's return value
    becomes `outs`.  warmup: run outside the capture first - True: the body itself, or a callable (the body and whatever puts back the
    state it changed); None where the caller has already run the sequence launch by launch.  The pins are taken BEFORE the capture begins
    and after the warm-up: were a workspace evicted between the warm-up and the capture, the body would otherwise allocate it inside
    torch.cuda.graph - in the graph's private pool - while the workspace cache holds it."""
    if warmup is not None:
        (body if warmup is True else warmup)()
    torch.cuda.synchronize()
    with holding(pins) as pinned, _collector_off():
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            outs = body()
    return Captured(graph, bufs, outs, pinned, {} if extra is None else extra)


@contextlib.contextmanager
def _collector_off():
    """No cyclic garbage collection while a capture is open.  A dead cycle may hold captured graphs (the frames of a call that raised keep
    its agents and samplers until the collector finds them, at whichever allocation crosses its threshold), and a graph's destructor
    synchronises the device: illegal during a capture and, failing inside a destructor, the end of the process.  Such garbage waits."""
    was_on = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_on:
            gc.enable()


class CapturedPasses(ShapeCache):
    """The captured passes of an encoder, per input shape, and the policy of its encode(): the first call of a shape runs launch by launch,
    the second captures, later ones replay."""

    def __init__(self, capacity):
        super().__init__(capacity, on_evict=release)
        self._seen_once = ShapeCache(4 * capacity)

    def entry(self, key, seen, make):
        """The entry of `key`, captured by make() if the shape was seen before; None: run this call launch by launch."""
        ent = self.get(key)
        if ent is None:
            if seen not in self._seen_once:
                # first call of a shape: launch by launch (a shape that never returns never pays a capture, and - kept apart from the
                # captured graphs - never evicts one: with more shapes in rotation than the cache holds, a shape is simply captured
                # again when it comes back, instead of every newcomer throwing out a live graph)
                self._seen_once[seen] = True
                return None
            ent = self[key] = make()
        return ent


class PinnedBlock:
    """One pinned host block and the event of the last copy out of it."""

    def __init__(self, shape, dtype=torch.float32):
        self.host = torch.zeros(shape, dtype=dtype).pin_memory()
        self._ev = torch.cuda.Event()  # (never recorded so far: the first synchronize() returns at once)

    def send(self, dst, fill, rows=None):
        """fill(block) writes the host block.  dst: the device tensor to overwrite, or a device - then a fresh tensor there.  The copy
        is in stream order on the current stream of dst's device; returns the device tensor.  rows: only the block's first `rows`
        entries along dim 0 travel (a block sized by capacity, a dst at least as long: its rest keeps what it held)."""
        self.wait()
        fill(self.host)
        src = self.host if rows is None else self.host[:rows]
        if torch.is_tensor(dst):
            (dst if rows is None else dst[:rows]).copy_(src, non_blocking=True)
        else:
            dst = src.to(dst, non_blocking=True)
        self._ev.record(torch.cuda.current_stream(dst.device))
        return dst

    def wait(self):
        self._ev.synchronize()  # the last copy out of the block has completed: the host may rewrite it, or let it go


class UploadRing:
    """`depth` slots of pinned blocks in rotation, for an owner that uploads the same few buffers on every call: advance() once per call,
    then send(name, ...) through the current slot's block of that name.  The host rewrites a block only `depth` calls after the copy out of
    it was issued, so the wait inside PinnedBlock.send finds that copy long completed and the host runs ahead of the device."""

    def __init__(self, depth, block=PinnedBlock):
        self.depth, self.slot, self._block, self._blocks = int(depth), 0, block, {}

    def advance(self):
        self.slot = (self.slot + 1) % self.depth

    def send(self, name, dst, fill, rows=None):
        """PinnedBlock.send through the block of (current slot, name): made on first use with dst's shape and dtype, and again when dst
        has been reallocated to another shape.  dst a device: through the block a send to a tensor has made (a device gives no shape)."""
        key = (self.slot, name)
        blk = self._blocks.get(key)
        if torch.is_tensor(dst) and (blk is None or blk.host.shape != dst.shape or blk.host.dtype != dst.dtype):
            if blk is not None:
                blk.wait()
            blk = self._blocks[key] = self._block(tuple(dst.shape), dst.dtype)
        return blk.send(dst, fill, rows)

    def drop(self, name):
        """Forgets every slot's block of `name` once the last copy out of each has completed (the device buffer is being reallocated)."""
        for key in [k for k in self._blocks if k[1] == name]:
            self._blocks.pop(key).wait()
