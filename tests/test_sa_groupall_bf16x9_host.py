"""CPU (no GPU): host side of the exact-product split-bf16 GroupAll kernel (csrc/sa_groupall_bf16x9.hip) - the packed weight stream against
pack_bf16x9's fragments and against the weights themselves, the all-or-nothing fallback of the level, the config field, and
gp_sa_groupall_bf16x9's declaration / export / ctypes signature."""
import ctypes

import pytest
import torch

from oracle import genpose_oracle as go
from sa_split_host import prototype


def _weights(c2, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(256, 512, generator=g), torch.randn(c2, 256, generator=g), torch.randn(512, c2, generator=g)


@pytest.mark.parametrize("c2", [256, 384])
def test_stream_is_pack_bf16x9s_fragments_in_ring_order(c2):
    from genpose_amd.weights import pack_bf16x9, pack_groupall_bf16x9
    W1, W2, W3 = _weights(c2)
    p = pack_groupall_bf16x9(W1, W2, W3)
    nh2, kb3 = c2 // 128, c2 // 32
    assert p.shape == (32 + 8 * nh2 + 4 * kb3, 8, 3, 64, 8) and p.dtype == torch.int16 and p.is_contiguous()
    f1, f2, f3 = pack_bf16x9(W1, 16, 16), pack_bf16x9(W2, 8 * nh2, 8), pack_bf16x9(W3, 32, kb3)  # [k-block][chunk][3][64][8]
    s = 0
    for h in range(2):
        for kb in range(16):                      # layer 1: output chunks 8 h .. 8 h + 7, k-blocks ascending
            assert torch.equal(p[s], f1[kb, 8 * h:8 * h + 8]), (h, kb)
            s += 1
        for kb in range(4 * h, 4 * h + 4):        # layer 2: k-blocks 4 h .. 4 h + 3, eight output chunks per slice
            for t in range(nh2):
                assert torch.equal(p[s], f2[kb, 8 * t:8 * t + 8]), (h, kb, t)
                s += 1
    for q in range(4):                            # layer 3: group of eight output chunks, k-blocks ascending
        for kb in range(kb3):
            assert torch.equal(p[s], f3[kb, 8 * q:8 * q + 8]), (q, kb)
            s += 1
    assert s == p.shape[0]
    with pytest.raises(ValueError):
        pack_groupall_bf16x9(W1[:, :256], W2, W3)
    with pytest.raises(ValueError):
        pack_groupall_bf16x9(W1, W2[:196], W3[:, :196])


@pytest.mark.parametrize("c2", [256, 384])
def test_the_three_terms_sum_to_the_weights_exactly(c2):
    from genpose_amd.weights import pack_groupall_bf16x9
    W1, W2, W3 = _weights(c2, seed=5)
    p = pack_groupall_bf16x9(W1, W2, W3)
    back = (p[:, :, 0].view(torch.bfloat16).double() + p[:, :, 1].view(torch.bfloat16).double()) + p[:, :, 2].view(torch.bfloat16).double()  # [slice][chunk][lane][8]
    nh2, kb3 = c2 // 128, c2 // 32
    lanes = torch.arange(64)
    n, g, e = lanes % 16, lanes // 16, torch.arange(8)
    koff = torch.where(e < 4, 4 * g[:, None] + e[None, :], 16 + 4 * g[:, None] + (e[None, :] - 4))  # [64, 8]: the chain's k order

    def element(W, chunk0, kb, sl):
        rows = 16 * (chunk0 + torch.arange(8))[:, None, None] + n[None, :, None]
        cols = (32 * kb + koff)[None].expand(8, 64, 8)
        assert torch.equal(back[sl], W.double()[rows.expand(8, 64, 8), cols]), sl

    s = 0
    for h in range(2):
        for kb in range(16):
            element(W1, 8 * h, kb, s)
            s += 1
        for kb in range(4 * h, 4 * h + 4):
            for t in range(nh2):
                element(W2, 8 * t, kb, s)
                s += 1
    for q in range(4):
        for kb in range(kb3):
            element(W3, 8 * q, kb, s)
            s += 1
    assert float(back.sum()) == pytest.approx(float(W1.double().sum() + W2.double().sum() + W3.double().sum()), rel=1e-9, abs=1e-9)  # every weight once


def test_level_pack_is_both_scales_or_nothing():
    from genpose_amd.weights import EncoderWeights, pack_groupall_bf16x9
    sd = go.make_state_dict(0, "score")
    w = EncoderWeights(sd, "cpu")
    stream, offs = w.groupall_bf16x9_packs()
    assert offs == [0, 80] and stream.shape == (184, 8, 3, 64, 8)
    for i, sc in enumerate(w.levels[3]):
        want = pack_groupall_bf16x9(sc.w1_feat, sc._folded_plain[1][0], sc._folded_plain[2][0])
        assert torch.equal(stream[offs[i]:offs[i] + want.shape[0]], want)
    for layer in (0, 1, 2):  # a subnormal entry in any one of the six matrices: the whole level keeps the fp32 kernels
        bad = dict(sd)
        key = f"pts_encoder.SA_modules.3.mlps.{layer % 2}.layer{layer}.conv.weight"
        W = bad[key].clone()
        W[3, 5] = 1e-40
        bad[key] = W
        assert EncoderWeights(bad, "cpu").groupall_bf16x9_packs() is None, key


def test_signature_matches_header_and_library_exports_it():
    from genpose_amd import _lib, build
    args = prototype("gp_sa_groupall_bf16x9")
    sig = _lib.SIGNATURES["gp_sa_groupall_bf16x9"]
    assert len(sig) == len(args) == 24
    for decl, ct in zip(args, sig):
        want = "pointer" if "*" in decl or decl.startswith("gp_stream_t") else "int"
        assert want == ("int" if ct is ctypes.c_int else "pointer"), (decl, ct)
    build.build()
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), "gp_sa_groupall_bf16x9")


def test_config_field_resolves_by_sampler():
    from genpose_amd.config import encoder_level3_of, encoder_precision_of, get_config
    assert get_config().encoder_level3 == "auto"
    assert encoder_level3_of(get_config(sampler_mode=["pc"])) == "bf16x9"
    for mode, steps in ((["ode"], None), (["heun"], 8), (["dpm2m"], 8)):
        assert encoder_level3_of(get_config(sampler_mode=mode, sampling_steps=steps)) == "f32mfma"
    assert encoder_level3_of(get_config(sampler_mode=["ode"], encoder_level3="bf16x9")) == "bf16x9"
    assert encoder_level3_of(get_config(sampler_mode=["pc"], encoder_level3="f32mfma")) == "f32mfma"
    assert encoder_precision_of(get_config(sampler_mode=["pc"], encoder_level3="f32mfma")) == "bf16x9"  # level 2's field is independent
    with pytest.raises(ValueError):
        encoder_level3_of(get_config(encoder_level3="fp8"))
