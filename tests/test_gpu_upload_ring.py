"""GPU: graphs.UploadRing with real pinned blocks.  The host runs ahead of the device here - nothing synchronises between the calls - so a
block that were rewritten before the copy out of it had completed, or a rotation that skipped the block's wait, would show as a clone
holding a later call's pattern."""
import pytest
import torch

from genpose_amd.graphs import UploadRing

pytestmark = pytest.mark.gpu

CALLS = 9


def test_every_call_of_a_depth_2_ring_delivers_its_own_pattern():
    dst = torch.zeros(64, dtype=torch.int32, device="cuda")
    patterns = [torch.arange(64, dtype=torch.int32) * (i + 1) + 1000 * i for i in range(CALLS)]
    ring, clones = UploadRing(2), []
    for p in patterns:
        ring.advance()
        assert ring.send("x", dst, lambda h: h.copy_(p)) is dst
        clones.append(dst.clone())  # (in stream order behind the copy)
    torch.cuda.synchronize()
    for i, (c, p) in enumerate(zip(clones, patterns)):
        assert torch.equal(c.cpu(), p), i
    assert len(ring._blocks) == 2 and all(blk.host.is_pinned() for blk in ring._blocks.values())


def test_rows_sends_the_first_rows_and_leaves_the_rest():
    keep = torch.arange(15, dtype=torch.float64).view(5, 3) - 100.0
    dst = keep.to("cuda")
    patterns = [torch.full((2, 3), i + 0.5, dtype=torch.float64) + torch.arange(3, dtype=torch.float64) for i in range(CALLS)]
    ring, clones = UploadRing(2), []
    for p in patterns:
        ring.advance()
        ring.send("x", dst, lambda h: h[:2].copy_(p), rows=2)
        clones.append(dst.clone())
    torch.cuda.synchronize()
    for i, (c, p) in enumerate(zip(clones, patterns)):
        assert torch.equal(c[:2].cpu(), p) and torch.equal(c[2:].cpu(), keep[2:]), i


def test_a_reallocated_dst_is_filled_whole_after_drop():
    ring = UploadRing(2)
    dst = torch.zeros(4, 2, device="cuda")
    for i in range(3):
        ring.advance()
        ring.send("x", dst, lambda h: h.fill_(float(i + 1)))
    ring.drop("x")
    assert not ring._blocks
    dst = torch.full((9, 2), -1.0, device="cuda")
    want = torch.arange(18, dtype=torch.float32).view(9, 2)
    ring.advance()
    ring.send("x", dst, lambda h: h.copy_(want))
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), want)
