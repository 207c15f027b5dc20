"""CPU (no GPU): layer 3's K tail of the exact-product split-bf16 level-2 kernel (csrc/sa_bf16x9.hip).  The kernel rebuilds the fp32
weights W3[:, 192:196] in its prologue from the packed stream: output channel c = 16 (8 h + n) + l sits in slice 8 + 7 h + 6 (slices 14
and 21), chunk n, lane l < 16 (lane group 0), elements e < 4 (k = 192 + e), as (hi + mid) + lo in float32.  Here the same positions and the
same two float32 additions on the host, for the seeded and the trained checkpoints: they give the folded weights back bit for bit."""
import os

import pytest
import torch

from oracle import genpose_oracle as go

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(ROOT, "tests", "golden", "trained", "ckpt_score.pth")


def tail_from_stream(stream):
    """[22][8][3][64][8] int16 -> [256, 4] float32: the kernel prologue's reads and arithmetic."""
    out = torch.empty(256, 4, dtype=torch.float32)
    for h in range(2):
        sl = stream[8 + 7 * h + 6]                                                  # [8 chunks][3][64][8]
        terms = sl[:, :, :16, :4].contiguous().view(torch.bfloat16).float()         # [n][t][l][e]
        v = (terms[:, 0] + terms[:, 1]) + terms[:, 2]                               # float32, in the kernel's order
        out[128 * h:128 * h + 128] = v.reshape(128, 4)                              # c - 128 h = 16 n + l
    return out


@pytest.mark.parametrize("name", ["seed0", "seed1", "trained"])
def test_tail_weights_come_back_from_the_stream_bit_for_bit(name):
    from genpose_amd.weights import EncoderWeights
    if name == "trained":
        assert os.path.exists(CKPT), f"{CKPT} is missing (committed fixture)"
        sd = {k: v.float() for k, v in torch.load(CKPT, map_location="cpu")["model_state_dict"].items()}
    else:
        sd = go.make_state_dict(int(name[-1]), "score")
    w = EncoderWeights(sd, "cpu")
    for sc in w.levels[2]:
        packs = sc.bf16x9_packs()
        assert packs is not None
        stream = packs[0]
        assert stream.shape == (22, 8, 3, 64, 8) and stream.dtype == torch.int16
        W3 = sc._folded_plain[2][0].float()
        assert W3.shape[0] == 256 and W3.shape[1] >= 196
        got = tail_from_stream(stream)
        assert torch.equal(got.view(torch.int32), W3[:, 192:196].contiguous().view(torch.int32))
        assert bool((got != 0).any())


def test_the_tail_slices_hold_nothing_else_of_the_real_weights():
    """Slices 14 and 21 beyond k = 195 are the zero k-padding of a 196-wide layer 3: what the kernel does not read there carries no weight."""
    from genpose_amd.weights import pack_sa_bf16x9
    g = torch.Generator().manual_seed(3)
    p = pack_sa_bf16x9(torch.randn(196, 128, generator=g), torch.randn(256, 196, generator=g))
    for s in (14, 21):
        assert bool(p[s, :, :, :16, :4].any())
        assert not bool(p[s, :, :, 16:].any()) and not bool(p[s, :, :, :16, 4:].any())
