"""Host side of genpose_amd/graphs.py without a device: the pin bookkeeping around a capture, its way back through every exit of a
ShapeCache, UploadRing's rotation over recording blocks, and that the pinned-upload protocol has one home."""
import os
import re

import pytest

from genpose_amd import graphs
from genpose_amd.lru import ShapeCache

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "genpose_amd")


def _takers(workspaces):
    return [lambda ws=ws: graphs.pin(ws) for ws in workspaces]


def test_a_capture_that_raises_leaves_every_pin_count_where_it_was():
    wss = [{}, {"_pins": 2}, {"_pins": 0}]
    with pytest.raises(KeyboardInterrupt):  # BaseException, not only Exception
        with graphs.holding(_takers(wss)) as pinned:
            assert [ws.get("_pins") for ws in wss] == [1, 3, 1] and all(a is b for a, b in zip(pinned, wss))
            raise KeyboardInterrupt
    assert [ws.get("_pins", 0) for ws in wss] == [0, 2, 0]
    assert graphs.unpinned(wss[0]) and not graphs.unpinned(wss[1])


def test_a_pin_that_cannot_be_taken_gives_the_earlier_ones_back():
    wss = [{}, {"_pins": 1}]

    def fails():
        raise MemoryError("no workspace")
    with pytest.raises(MemoryError):
        with graphs.holding(_takers(wss) + [fails]):
            pytest.fail("the block must not run")
    assert [ws.get("_pins", 0) for ws in wss] == [0, 1]


def test_a_capture_that_succeeds_leaves_each_count_one_higher():
    wss = [{}, {"_pins": 2}]
    with graphs.holding(_takers(wss)) as pinned:
        pass
    assert [ws["_pins"] for ws in wss] == [1, 3] and pinned == wss
    graphs.release("key", graphs.Captured(None, (), None, pinned, {}))
    assert [ws["_pins"] for ws in wss] == [0, 2]


def _entry(*workspaces):
    with graphs.holding(_takers(workspaces)) as pinned:
        return graphs.Captured(None, (), None, pinned, {})


def test_release_returns_the_pins_on_every_way_out_of_a_cache():
    """The four ways out that lru.ShapeCache has: eviction, overwrite, pop and clear."""
    ws = [{} for _ in range(5)]
    cache = ShapeCache(2, on_evict=graphs.release)
    cache["a"] = _entry(ws[0], ws[4])
    cache["b"] = _entry(ws[1], ws[4])
    assert [w["_pins"] for w in ws[:2]] == [1, 1] and ws[4]["_pins"] == 2
    cache["c"] = _entry(ws[2])  # evicts "a", the least recently used
    assert "a" not in cache and ws[0]["_pins"] == 0 and ws[4]["_pins"] == 1 and ws[1]["_pins"] == 1
    cache["c"] = _entry(ws[3])  # overwrites
    assert ws[2]["_pins"] == 0 and ws[3]["_pins"] == 1
    same = cache["c"]
    cache["c"] = same  # (the same entry again is no way out)
    assert ws[3]["_pins"] == 1
    assert cache.pop("b") is not None and ws[1]["_pins"] == 0 and ws[4]["_pins"] == 0
    cache.clear()
    assert len(cache) == 0 and all(graphs.unpinned(w) for w in ws)


def test_captured_passes_run_a_shape_direct_once_then_capture_then_keep():
    made = []

    def make(ws):
        made.append(ws)
        return _entry(ws)
    ws = [{} for _ in range(4)]
    passes = graphs.CapturedPasses(2)
    assert passes.entry("k0", "s0", lambda: make(ws[0])) is None and not made  # seen once: launch by launch, nothing captured
    e0 = passes.entry("k0", "s0", lambda: make(ws[0]))
    assert e0 is not None and made == [ws[0]] and ws[0]["_pins"] == 1
    assert passes.entry("k0", "s0", lambda: make(ws[0])) is e0 and len(made) == 1  # later calls: the same entry
    for i in (1, 2):  # two more shapes: the first of them never evicts a live graph, the capture of the second evicts the oldest
        assert passes.entry(f"k{i}", f"s{i}", lambda: make(ws[i])) is None and len(passes) == i and "k0" in passes
        passes.entry(f"k{i}", f"s{i}", lambda: make(ws[i]))
    assert len(passes) == 2 and "k0" not in passes and ws[0]["_pins"] == 0
    assert passes.entry("k0", "s0", lambda: make(ws[3])) is not None  # a shape that comes back is captured again at once
    passes.clear()
    assert all(graphs.unpinned(w) for w in ws)


def _code(name):
    with open(os.path.join(PKG, name)) as f:
        return f.read()


def test_the_pinned_upload_protocol_and_the_pin_count_have_one_home():
    """PinnedBlock needs a device to allocate its block, so what is checked here is that the conversion left no second copy: pinned host
    memory is allocated in samplers.py only for ODESampler's blocking read-backs (_tables_host, _state_host), in posenet.py nowhere, and
    the count `_pins` is written by graphs.pin / graphs.unpin alone.  Over the whole package: no other module allocates pinned memory or
    touches a block's event, and the seed state's words are masked together nowhere but in _lib.seed_words' callers' arguments."""
    pinned = {name: re.findall(r"^.*\.pin_memory\(\).*$", _code(name), re.M) for name in ("samplers.py", "posenet.py")}
    assert pinned["posenet.py"] == []
    assert len(pinned["samplers.py"]) == 2 and all("self._tables_host = " in l or "self._state_host = " in l for l in pinned["samplers.py"])
    writes = {}
    for name in sorted(os.listdir(PKG)):
        if name.endswith(".py"):
            found = re.findall(r"""\[["']_pins["']\]\s*(?:=(?!=)|[-+]=)""", _code(name))
            if found:
                writes[name] = len(found)
    assert writes == {"graphs.py": 2}
    graph_sites = {name: _code(name).count("torch.cuda.CUDAGraph(") for name in sorted(os.listdir(PKG)) if name.endswith(".py")}
    assert {k: v for k, v in graph_sites.items() if v} == {"graphs.py": 1}
    # the whole package: the front ends, the tracker and the pipeline's prior uploads go through PinnedBlock / UploadRing as well, the
    # block's event is graphs.py's own, and the seed state's words are assembled by _lib.seed_words alone
    modules = [name for name in sorted(os.listdir(PKG)) if name.endswith(".py")]
    assert {name for name in modules if ".pin_memory()" in _code(name)} == {"graphs.py", "samplers.py"}
    assert {name for name in modules if re.search(r"\b_ev\b", _code(name))} == {"graphs.py"}
    assert "0xFFFFFFFF" not in _code("runner.py") and "0xFFFFFFFF" not in _code("samplers.py")
    # preprocess.py: the Philox reference (_philox_word0, seeded_ranks), frame_tables' draw table, the front ends' slot_base - nowhere else
    masks = [line.strip() for line in _code("preprocess.py").splitlines() if "0xFFFFFFFF" in line]
    allowed = ("m0, m1, sh, lo32 = ", "u32 = lambda v: ", "draw = np.array([(int(runs[f]) & 0xFFFFFFFF, int(s) & 0xFFFFFFFF)")
    assert len(masks) == 4 and all(line.startswith(allowed) or "int(slot_base) & 0xFFFFFFFF" in line for line in masks)
    assert sum("int(slot_base) & 0xFFFFFFFF" in line for line in masks) == 1 and all(line.count("0xFFFFFFFF") == 1 for line in masks if not line.startswith(allowed))


def _recording_ring(depth):
    """An UploadRing over host-only blocks that record what happens to them -> (ring, the blocks in the order they were made)."""
    import torch
    made = []

    class Block:
        def __init__(self, shape, dtype):
            self.host, self.sent, self.waits = torch.zeros(shape, dtype=dtype), [], 0
            made.append(self)

        def send(self, dst, fill, rows=None):
            fill(self.host)
            self.sent.append((dst, rows))
            return dst

        def wait(self):
            self.waits += 1
    return graphs.UploadRing(depth, block=Block), made


def test_the_ring_rotates_once_per_advance_and_makes_each_block_once():
    """Depth 3, two names, seven calls of an owner: advance() comes first in a call, so the slots go 1, 2, 0, 1, 2, 0, 1."""
    import torch
    ring, made = _recording_ring(3)
    a, b = torch.zeros(4, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.float64)
    slots, blocks = [], {}
    for call in range(7):
        ring.advance()
        slots.append(ring.slot)
        for name, dst in (("a", a), ("b", b)):
            n_before = len(made)
            assert ring.send(name, dst, lambda h: h.fill_(call)) is dst
            blk = ring._blocks[(ring.slot, name)]
            assert blk.sent[-1] == (dst, None) and blk.host.shape == dst.shape and blk.host.dtype == dst.dtype and bool((blk.host == call).all())
            assert (len(made) == n_before + 1) == (call < 3)  # made in the slot's first call, found again afterwards
            assert blocks.setdefault((ring.slot, name), blk) is blk
    assert slots == [1, 2, 0, 1, 2, 0, 1]
    assert len(made) == 6 == len(blocks) and len({id(blk) for blk in made}) == 6
    assert sorted(len(blk.sent) for blk in made) == [2, 2, 2, 2, 3, 3]  # slot 1 served three calls, slots 2 and 0 two each
    # rows= goes through to the block as it is
    ring.send("a", a, lambda h: None, rows=2)
    assert ring._blocks[(ring.slot, "a")].sent[-1] == (a, 2)
    # a dst of another shape: that name's block of the slot in use is made again (after a wait for the old one), no other block is
    old, others = ring._blocks[(ring.slot, "a")], [blk for key, blk in ring._blocks.items() if key != (ring.slot, "a")]
    a9 = torch.zeros(9, dtype=torch.int32)
    ring.send("a", a9, lambda h: h.fill_(5))
    new = ring._blocks[(ring.slot, "a")]
    assert new is not old and old.waits == 1 and new.host.shape == (9,) and len(made) == 7
    assert [blk for key, blk in ring._blocks.items() if key != (ring.slot, "a")] == others and all(blk.waits == 0 for blk in others)
    ring.send("a", a9, lambda h: None)
    assert ring._blocks[(ring.slot, "a")] is new and len(made) == 7
    # ... and of another dtype
    ring.send("a", a9.to(torch.int64), lambda h: None)
    assert ring._blocks[(ring.slot, "a")].host.dtype == torch.int64 and len(made) == 8


def test_the_first_send_of_an_owner_needs_no_advance():
    import torch
    ring, made = _recording_ring(2)
    dst = torch.zeros(3)
    assert ring.send("x", dst, lambda h: h.fill_(1.0)) is dst and ring.slot == 0 and len(made) == 1 and bool((made[0].host == 1).all())


def test_drop_waits_for_every_block_of_the_name_and_for_no_other():
    import torch
    ring, made = _recording_ring(3)
    a, b = torch.zeros(4), torch.zeros(5)
    for _ in range(3):
        ring.advance()
        ring.send("a", a, lambda h: None)
        ring.send("b", b, lambda h: None)
    blocks_a = [blk for (slot, name), blk in ring._blocks.items() if name == "a"]
    blocks_b = [blk for (slot, name), blk in ring._blocks.items() if name == "b"]
    assert len(blocks_a) == 3 == len(blocks_b)
    ring.drop("a")
    assert [blk.waits for blk in blocks_a] == [1, 1, 1] and [blk.waits for blk in blocks_b] == [0, 0, 0]
    assert sorted(ring._blocks) == [(0, "b"), (1, "b"), (2, "b")]
    ring.drop("a")  # (nothing of that name: nothing happens)
    assert [blk.waits for blk in blocks_a] == [1, 1, 1]
    ring.send("a", torch.zeros(9), lambda h: None)  # the reallocated buffer's first send makes the slot's block anew
    assert ring._blocks[(ring.slot, "a")].host.shape == (9,) and len(made) == 7


def test_no_cyclic_collection_while_a_capture_is_open():
    """capture() wraps the capture in graphs._collector_off: a dead cycle that holds a graph must not be collected inside a capture (the
    graph's destructor synchronises the device).  The collector's state comes back as it was, also when the body raises."""
    import gc
    assert gc.isenabled()
    with graphs._collector_off():
        assert not gc.isenabled()
    assert gc.isenabled()
    with pytest.raises(KeyboardInterrupt):
        with graphs.holding([]), graphs._collector_off():
            raise KeyboardInterrupt
    assert gc.isenabled()
    gc.disable()
    try:
        with graphs._collector_off():
            pass
        assert not gc.isenabled()  # it was off before: it stays off
    finally:
        gc.enable()
