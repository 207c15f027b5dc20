"""Host side of the exact-product split-bf16 trunk (csrc/trunk_bf16x9.hip): the weight split hi + mid + lo == W holds bit for bit on every
weight of the seeded and the trained checkpoints, the packed fragments follow pack_bf16x3's order, and a weight that cannot be split
exactly is refused at pack time."""
import os

import pytest
import torch

from oracle import genpose_oracle as go

HERE = os.path.dirname(os.path.abspath(__file__))
CKPT = os.path.join(HERE, "golden", "trained", "ckpt_score.pth")


def _trunk_weights(sd, prefix="pose_score_net."):
    heads = ("rot_x", "rot_y", "trans")
    W1 = torch.cat([sd[f"{prefix}fusion_tail_{h}.0.weight"].float() for h in heads], dim=0)
    return {"pose0": sd[prefix + "pose_encoder.0.weight"].float(), "pose2": sd[prefix + "pose_encoder.2.weight"].float(),
            "headx": W1[:, 1152:1408].contiguous()}


def _checkpoints():
    out = {f"seed{s}": go.make_state_dict(s, "score") for s in (0, 1, 2)}
    if os.path.exists(CKPT):
        out["trained"] = {k: v.float() for k, v in torch.load(CKPT, map_location="cpu")["model_state_dict"].items()}
    return out


@pytest.mark.parametrize("name", ["seed0", "seed1", "seed2", "trained"])
def test_split_is_exact_on_every_trunk_weight(name):
    from genpose_amd.weights import pack_bf16x3, pack_bf16x9, split_bf16x9
    sds = _checkpoints()
    assert name in sds, f"{CKPT} is missing (committed fixture)"
    for key, W in _trunk_weights(sds[name]).items():
        hi, mid, lo = split_bf16x9(W)
        assert torch.equal((hi.double() + mid.double()) + lo.double(), W.double()), (name, key)
        # the terms shrink by at least 2^8 each: hi carries the leading eight bits
        nz = mid.float() != 0
        assert bool((mid.float().abs()[nz] <= hi.float().abs()[nz] * 2.0 ** -8).all()), (name, key)
        chain = key != "pose0"
        nc, kb = (16, 1) if key == "pose0" else ((16, 8) if key == "pose2" else (48, 8))
        p9, p3 = pack_bf16x9(W, nc, kb, chain=chain), pack_bf16x3(W, nc, kb, chain=chain)
        assert p9.shape == (kb, nc, 3, 64, 8) and p9.dtype == torch.int16
        assert torch.equal(p9[:, :, 0], p3[:, :, 0])  # hi: the same fragments as the hi part of the bf16x3 pack
        back = sum(p9[:, :, t].view(torch.bfloat16).double() for t in range(3))
        ref = sum(p3[:, :, t].view(torch.bfloat16).double() for t in range(2))
        assert float((back - ref).abs().max()) <= float(ref.abs().max()) * 2.0 ** -16  # bf16x3 drops only the lo term's share


def test_split_refuses_what_it_cannot_represent():
    from genpose_amd.weights import pack_bf16x9, split_bf16x9
    W = torch.randn(32, 32)
    split_bf16x9(W)
    for bad in (float("nan"), float("inf"), 1e-38 * (1 + 2.0 ** -20)):  # the last one's mid / lo terms fall below the normal range
        Wb = W.clone()
        Wb[3, 5] = bad
        with pytest.raises(ValueError):
            pack_bf16x9(Wb, 2, 1)


def _slow_pack(terms, n_out, k_in, n_chunks, k_blocks, chain):
    """The docstrings' definition, one element at a time: out[kb][nc][t][lane][e] = term t of W[16 nc + n][32 kb + koff(g, e)] with
    lane = (n = lane % 16, g = lane // 16), koff = 4 g + e (e < 4) or 16 + 4 g + e - 4 for the register chain's k order, 8 g + e for
    the natural one; zero outside W."""
    out = torch.zeros(k_blocks, n_chunks, len(terms), 64, 8, dtype=torch.int16)
    for kb in range(k_blocks):
        for nc in range(n_chunks):
            for lane in range(64):
                n, g = lane % 16, lane // 16
                for e in range(8):
                    koff = (4 * g + e if e < 4 else 16 + 4 * g + e - 4) if chain else 8 * g + e
                    r, c = 16 * nc + n, 32 * kb + koff
                    if r < n_out and c < k_in:
                        for t, term in enumerate(terms):
                            out[kb, nc, t, lane, e] = term[r, c]
    return out


@pytest.mark.parametrize("shape,nc,kb,chain", [((768, 256), 48, 8, True), ((256, 9), 16, 1, False), ((37, 70), 3, 3, True)])
def test_packs_match_the_per_element_definition(shape, nc, kb, chain):
    from genpose_amd.weights import pack_bf16x3, pack_bf16x9, split_bf16x9
    W = torch.randn(*shape, generator=torch.Generator().manual_seed(7))
    hi = W.to(torch.bfloat16)
    lo = (W - hi.float()).to(torch.bfloat16)
    p3 = pack_bf16x3(W, nc, kb, chain=chain)
    assert p3.shape == (kb, nc, 2, 64, 8) and p3.dtype == torch.int16 and p3.is_contiguous()
    assert torch.equal(p3, _slow_pack([t.view(torch.int16) for t in (hi, lo)], *shape, nc, kb, chain))
    p9 = pack_bf16x9(W, nc, kb, chain=chain)
    assert p9.shape == (kb, nc, 3, 64, 8) and p9.dtype == torch.int16 and p9.is_contiguous()
    assert torch.equal(p9, _slow_pack([t.view(torch.int16) for t in split_bf16x9(W)], *shape, nc, kb, chain))
