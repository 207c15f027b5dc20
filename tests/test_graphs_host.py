"""Host side of genpose_amd/graphs.py without a device: the pin bookkeeping around a capture, its way back through every exit of a
ShapeCache, and that the pinned-upload protocol has one home."""
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
    the count `_pins` is written by graphs.pin / graphs.unpin alone."""
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
