"""CPU (no GPU): host side of the exact-product split-bf16 level-2 kernel (csrc/sa_bf16x9.hip) - the packed weight stream against its
per-element definition, the exactness of the split on the level-2 weights of the seeded and trained checkpoints, the refusal of a weight
that does not split, and gp_sa_pre_mlp_max_bf16x9's declaration / export / ctypes signature."""
import ctypes
import os

import pytest
import torch

from oracle import genpose_oracle as go
from sa_split_host import prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(ROOT, "tests", "golden", "trained", "ckpt_score.pth")


def _slow_stream(W2, W3):
    """The definition, one element at a time: out[s][c][t][lane][e] = term t of W[16 nc + lane % 16][32 kb + koff] with koff = 4 g + e (e < 4)
    or 16 + 4 g + e - 4, g = lane // 16; slice s < 8: W = W2, kb = s // 2, nc = 8 (s % 2) + c; s >= 8: W = W3, nc = 8 ((s - 8) // 7) + c,
    kb = (s - 8) % 7; zero outside W."""
    from genpose_amd.weights import split_bf16x9
    t2, t3 = [t.view(torch.int16) for t in split_bf16x9(W2)], [t.view(torch.int16) for t in split_bf16x9(W3)]
    out = torch.zeros(22, 8, 3, 64, 8, dtype=torch.int16)
    for s in range(22):
        terms, kb, h = (t2, s // 2, s % 2) if s < 8 else (t3, (s - 8) % 7, (s - 8) // 7)
        for c in range(8):
            for lane in range(64):
                n, g = lane % 16, lane // 16
                for e in range(8):
                    r, col = 16 * (8 * h + c) + n, 32 * kb + (4 * g + e if e < 4 else 16 + 4 * g + e - 4)
                    if r < terms[0].shape[0] and col < terms[0].shape[1]:
                        for t in range(3):
                            out[s, c, t, lane, e] = terms[t][r, col]
    return out


@pytest.mark.parametrize("k3", [196, 224])
def test_stream_matches_the_per_element_definition(k3):
    from genpose_amd.weights import pack_sa_bf16x9
    g = torch.Generator().manual_seed(11)
    W2, W3 = torch.randn(196, 128, generator=g), torch.randn(256, k3, generator=g)
    p = pack_sa_bf16x9(W2, W3)
    assert p.shape == (22, 8, 3, 64, 8) and p.dtype == torch.int16 and p.is_contiguous()
    assert torch.equal(p, _slow_stream(W2, W3))
    # the padding: output chunks 13-15 of layer 2 (slices 2 kb + 1, chunks 5-7) are zero
    assert not bool(p[1:8:2, 5:].any())
    with pytest.raises(ValueError):
        pack_sa_bf16x9(W2[:, :96], W3)


@pytest.mark.parametrize("name", ["seed0", "seed1", "trained"])
def test_level2_weights_of_the_checkpoints_split_exactly(name):
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
        stream, b2p, b3 = packs
        (_, _), (W2, b2), (W3, b3f) = sc._folded_plain
        back = sum(stream[:, :, t].view(torch.bfloat16).double() for t in range(3))  # hi + mid + lo of every packed element
        assert float(back.abs().max()) == float(max(W2.abs().max(), W3.abs().max()))
        assert float(back.sum()) == pytest.approx(float(W2.double().sum() + W3.double().sum()), rel=1e-9, abs=1e-9)  # every weight exactly once
        assert torch.equal(b2p[:196], b2) and not bool(b2p[196:].any()) and b2p.numel() == 224 and torch.equal(b3, b3f)


def test_a_weight_that_does_not_split_gives_no_pack():
    from genpose_amd.weights import EncoderWeights
    sd = dict(go.make_state_dict(0, "score"))
    key = "pts_encoder.SA_modules.2.mlps.1.layer2.conv.weight"
    W = sd[key].clone()
    W[3, 5] = 1e-40
    sd[key] = W
    w = EncoderWeights(sd, "cpu")
    assert w.levels[2][1].bf16x9_packs() is None and w.levels[2][0].bf16x9_packs() is not None


def test_signature_matches_header_and_is_the_bf16x3_one_with_one_weight_stream():
    from genpose_amd import _lib
    args = prototype("gp_sa_pre_mlp_max_bf16x9")
    sig = _lib.SIGNATURES["gp_sa_pre_mlp_max_bf16x9"]
    assert len(sig) == len(args)
    for decl, ct in zip(args, sig):
        want = "pointer" if "*" in decl or decl.startswith("gp_stream_t") else "int"
        assert want == ("int" if ct is ctypes.c_int else "pointer"), (decl, ct)
    x3 = prototype("gp_sa_pre_mlp_max_bf16x3")
    assert args == [a.replace("w2_split", "w23_x9") for a in x3 if a != "const void *w3_split"]


def test_library_exports_it_and_config_default():
    from genpose_amd import _lib, build
    from genpose_amd.config import encoder_precision_of, get_config
    build.build()
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), "gp_sa_pre_mlp_max_bf16x9")
    assert get_config().encoder_level2 == "auto"
    assert encoder_precision_of(get_config(sampler_mode=["pc"])) == "bf16x9"  # the fixed-step sampler: the split kernel by default
    assert encoder_precision_of(get_config(sampler_mode=["ode"])) == "f32"    # the adaptive solver keeps the fp32 kernels unless asked
    assert encoder_precision_of(get_config(sampler_mode=["ode"], encoder_level2="bf16x9")) == "bf16x9"
    assert encoder_precision_of(get_config(sampler_mode=["pc"], encoder_level2="f32mfma")) == "f32"
    assert encoder_precision_of(get_config(sampler_mode=["pc"], encoder_precision="bf16x3")) == "bf16x3"
    with pytest.raises(ValueError):
        encoder_precision_of(get_config(encoder_level2="fp8"))
