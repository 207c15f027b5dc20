"""GPU: layer 3's K tail of the exact-product split-bf16 level-2 kernel (csrc/sa_bf16x9.hip).  The hidden layer is 196 = 6 x 32 + 4 wide:
six k-blocks of layer 3 go through the BF16 ring, hidden channels 192-195 as one v_mfma_f32_16x16x4_f32 per (output chunk, tile) on fp32
weights rebuilt from slices 14 / 21 of the packed stream.  Through the C entry point, level 2's shapes (256 source points x 128 hoisted
channels per scale, 128 centres, ns = 16 | 32, 1 and 3 clouds; synthetic coordinates, indices and features):

- each tail k reaches the output through its own lane group and weight, bit for bit (an exact product: the expected value is closed form);
- the tail is the only path of those channels;
- a cloud's bits do not depend on its position in the batch or on capture + replay;
- what the kernel must not read (layer-3 columns >= 196, the rest of slices 14 / 21) never reaches the output."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

NB = 3
NSS = (16, 32)  # scale i of level 2


@functools.lru_cache(maxsize=None)
def _inputs():
    """Three clouds of level-2 inputs, read-only: coordinates, centres, neighbour indices per scale, hoisted features, layer 1."""
    g = torch.Generator().manual_seed(196)
    xyz = torch.rand(NB, 256, 3, generator=g)
    ins = {"xyz": xyz.cuda(), "new_xyz": xyz[:, :128].contiguous().cuda(), "z": torch.randn(NB, 256, 256, generator=g).cuda(),
           "idx": [torch.randint(0, 256, (NB, 128, ns), generator=g, dtype=torch.int32).cuda() for ns in NSS],
           "wxyz": (0.5 * torch.randn(128, 4, generator=g)).cuda(), "b1": (0.1 * torch.randn(128, generator=g)).cuda()}
    return ins


def _cloud(ins, c):
    return {k: ([t[c:c + 1].contiguous() for t in v] if k == "idx" else v[c:c + 1].contiguous() if k in ("xyz", "new_xyz", "z") else v) for k, v in ins.items()}


def _run(i, ins, B, packs, out=None, sync=True):
    """Scale i of level 2 for the first B clouds through gp_sa_pre_mlp_max_bf16x9; -> [B, 128, 256]."""
    from genpose_amd import _lib
    from genpose_amd._lib import ptr, stream_ptr
    ns = ins["idx"][i].shape[-1]
    if out is None:
        out = torch.full((B, 128, 512), float("nan"), device="cuda")
    w, b2p, b3p = packs
    _lib.call("gp_sa_pre_mlp_max_bf16x9", B, 256, 128, ns, 128, 196, 256, ptr(ins["xyz"]), ptr(ins["new_xyz"]), ptr(ins["idx"][i]), ptr(ins["z"]), 256, 128 * i,
              ptr(ins["wxyz"]), ptr(ins["b1"]), ptr(w), ptr(b2p), ptr(b3p), ptr(out), 512, 256 * i, stream_ptr())
    if not sync:
        return out
    torch.cuda.synchronize()
    other = out[..., 256 * (1 - i):256 * (1 - i) + 256]
    assert bool(torch.isnan(other).all())  # the other scale's columns are not touched
    return out[..., 256 * i:256 * i + 256].clone()


def _full_significands(e):
    """256 positive weights in [1, 2) with all 24 significand bits in use (the lowest one set), different for every channel and e."""
    j = (torch.arange(256, dtype=torch.int64) * 2654435761 + 40503 * (e + 1)) % (1 << 23) | 1
    w = (1.0 + j.double() * 2.0 ** -23).float()
    assert torch.equal(w.double(), 1.0 + j.double() * 2.0 ** -23) and w.unique().numel() == 256
    return w


def _one_k_packs(e, keep=True):
    """W2 = 0, W3 = 0 but column 192 + e, b2[192 + e] = 2^e, every other bias 0: the hidden layer is the constant 2^e at channel 192 + e."""
    from genpose_amd.weights import pack_sa_bf16x9
    W3 = torch.zeros(256, 196)
    wcol = _full_significands(e)
    if keep:
        W3[:, 192 + e] = wcol
    b2p = torch.zeros(224)
    b2p[192 + e] = 2.0 ** e
    return (pack_sa_bf16x9(torch.zeros(196, 128), W3).cuda(), b2p.cuda(), torch.zeros(256).cuda()), wcol * 2.0 ** e


@functools.lru_cache(maxsize=None)
def _random_packs():
    from genpose_amd.weights import pack_sa_bf16x9
    g = torch.Generator().manual_seed(7)
    W2, W3 = torch.randn(196, 128, generator=g) / 128 ** 0.5, torch.randn(256, 196, generator=g) / 14
    b2p = torch.zeros(224)
    b2p[:196] = 0.1 * torch.randn(196, generator=g)
    b3 = 0.1 * torch.randn(256, generator=g)
    return W2, W3, b2p, b3, (pack_sa_bf16x9(W2, W3).cuda(), b2p.cuda(), b3.cuda())


@pytest.mark.parametrize("e", range(4))
def test_each_tail_k_lands_in_its_lane_group_bit_for_bit(e):
    ins = _inputs()
    packs, want = _one_k_packs(e)
    for i in range(2):
        for B in (1, 3):
            out = _run(i, ins, B, packs)
            assert torch.equal(out.cpu().view(torch.int32), want.expand(B, 128, 256).contiguous().view(torch.int32)), (e, NSS[i], B)


@pytest.mark.parametrize("e", range(4))
def test_the_tail_is_the_only_path_for_those_channels(e):
    ins = _inputs()
    packs, _ = _one_k_packs(e, keep=False)
    for i in range(2):
        for B in (1, 3):
            out = _run(i, ins, B, packs)
            assert not bool(out.view(torch.int32).any()), (e, NSS[i], B)  # +0.0 everywhere


def test_a_clouds_bits_do_not_depend_on_its_position():
    ins = _inputs()
    packs = _random_packs()[4]
    for i in range(2):
        three = _run(i, ins, 3, packs)
        one = _run(i, _cloud(ins, 2), 1, packs)
        assert not bool(torch.isnan(three).any()) and bool((three > 0).any())
        assert torch.equal(three[2], one[0]), NSS[i]
        assert torch.equal(three[:1], _run(i, ins, 1, packs)), NSS[i]


def test_capture_and_replay_give_the_launched_bits():
    ins = _inputs()
    packs = _random_packs()[4]
    for i in range(2):
        direct = _run(i, ins, 3, packs)
        out = torch.full((3, 128, 512), float("nan"), device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _run(i, ins, 3, packs, out=out, sync=False)
        for _ in range(2):  # capture + replay, then a second replay
            out.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out[..., 256 * i:256 * i + 256], direct), NSS[i]
            assert bool(torch.isnan(out[..., 256 * (1 - i):256 * (1 - i) + 256]).all())


def test_what_is_not_read_never_reaches_the_output():
    from genpose_amd.weights import pack_sa_bf16x9
    ins = _inputs()
    W2, W3, b2p, b3, clean = _random_packs()
    g = torch.Generator().manual_seed(5)
    wide = pack_sa_bf16x9(W2, torch.cat([W3, 1e3 * torch.randn(256, 28, generator=g)], dim=1)).cuda()  # columns 196-223
    nans = clean[0].clone()
    for s in (14, 21):  # everything of the tail slices but lanes 0-15, elements 0-3: quiet-NaN bit patterns
        nans[s, :, :, 16:, :] = 0x7FC0
        nans[s, :, :, :16, 4:] = 0x7FC0
    assert not torch.equal(wide, clean[0]) and not torch.equal(nans, clean[0])
    no_tail = W3.clone()
    no_tail[:, 192:196] = 0
    zeroed = pack_sa_bf16x9(W2, no_tail).cuda()
    for i in range(2):
        for B in (1, 3):
            a = _run(i, ins, B, clean)
            assert not bool(torch.isnan(a).any())
            assert torch.equal(a, _run(i, ins, B, (wide, clean[1], clean[2]))), (NSS[i], B)
            assert torch.equal(a, _run(i, ins, B, (nans, clean[1], clean[2]))), (NSS[i], B)
            assert not torch.equal(a, _run(i, ins, B, (zeroed, clean[1], clean[2]))), (NSS[i], B)  # the tail itself does count
