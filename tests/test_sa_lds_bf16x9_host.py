"""CPU (no GPU): host side of the LDS-resident exact-product split-bf16 level-1 kernel (csrc/sa_lds_bf16x9.hip) - the per-scale packs against
the weights themselves in pack_bf16x9's k order, the per-scale fallback, the config field, and gp_sa_lds_bf16x9's declaration / export /
ctypes signature."""
import ctypes

import pytest
import torch

from oracle import genpose_oracle as go
from sa_split_host import k_of, prototype, terms

C2 = (64, 96)


def test_packs_have_the_documented_shapes_and_hold_the_three_terms_in_k_order():
    from genpose_amd.weights import EncoderWeights
    w = EncoderWeights(go.make_state_dict(0, "score"), "cpu")
    for i, sc in enumerate(w.levels[1]):
        assert tuple(sc.couts) == (64, C2[i], 128)
        w2, b2, w3, b3 = sc.bf16x9_lds_packs()
        assert sc.bf16x9_lds_packs()[0] is w2  # packed once
        (_, _), (W2, B2), (W3, B3) = sc._folded_plain
        assert w2.shape == (2, C2[i] // 16, 3, 64, 8) and w3.shape == (C2[i] // 32, 8, 3, 64, 8)
        assert w2.dtype == w3.dtype == torch.int16 and w2.is_contiguous() and w3.is_contiguous()
        assert b2.shape == (C2[i],) and b3.shape == (128,) and torch.equal(b2, B2.float()) and torch.equal(b3, B3.float())
        for pack, W in ((w2, W2), (w3, W3)):
            hml = terms(W.float())
            nkb, nch = pack.shape[0], pack.shape[1]
            # spot checks: all four lane groups, both halves of a k-block (e < 4, e >= 4), first / last k-block and chunk
            for kb in (0, nkb - 1):
                for nc in (0, nch // 2, nch - 1):
                    for lane in (0, 5, 16 + 9, 32 + 15, 48 + 2, 63):
                        n, g = lane % 16, lane // 16
                        for e in (0, 3, 4, 7):
                            for t in range(3):
                                want = hml[t][16 * nc + n, k_of(kb, g, e)].view(torch.int16)
                                assert pack[kb, nc, t, lane, e] == want, (kb, nc, t, lane, e)
            # and whole: the three terms of every fragment element sum to the weight pack_bf16x9's k order names, each weight once
            back = (pack[:, :, 0].view(torch.bfloat16).double() + pack[:, :, 1].view(torch.bfloat16).double()) + pack[:, :, 2].view(torch.bfloat16).double()
            lanes, e = torch.arange(64), torch.arange(8)
            n, g = lanes % 16, lanes // 16
            koff = torch.where(e < 4, 4 * g[:, None] + e[None, :], 16 + 4 * g[:, None] + (e[None, :] - 4))
            rows = (16 * torch.arange(nch)[None, :, None, None] + n[None, None, :, None]).expand(nkb, nch, 64, 8)
            cols = (32 * torch.arange(nkb)[:, None, None, None] + koff[None, None]).expand(nkb, nch, 64, 8)
            assert torch.equal(back, W.double()[rows, cols])
            assert back.numel() == W.numel()


def test_subnormal_weight_gives_none_for_that_scale_only():
    from genpose_amd.weights import EncoderWeights
    sd = go.make_state_dict(0, "score")
    for layer in (1, 2):
        bad = dict(sd)
        key = f"pts_encoder.SA_modules.1.mlps.0.layer{layer}.conv.weight"
        W = bad[key].clone()
        W[3, 5] = 1e-40
        bad[key] = W
        w = EncoderWeights(bad, "cpu")
        assert w.levels[1][0].bf16x9_lds_packs() is None and w.levels[1][0].bf16x9_lds_packs() is None, key
        assert w.levels[1][1].bf16x9_lds_packs() is not None
    # widths that are not whole k-blocks (level 2's 196) have no such pack
    assert EncoderWeights(sd, "cpu").levels[2][0].bf16x9_lds_packs() is None


def test_signature_matches_header_and_library_exports_it():
    from genpose_amd import _lib, build
    args = prototype("gp_sa_lds_bf16x9")
    sig = _lib.SIGNATURES["gp_sa_lds_bf16x9"]
    assert len(sig) == len(args) == 23
    names = [a.split()[-1].lstrip("*") for a in args]
    assert names == ["b", "n", "np", "ns", "c1", "c2", "c3", "xyz", "new_xyz", "idx", "z", "zstride", "zoff", "wxyz", "bias1", "w2_x9", "bias2", "w3_x9",
                     "bias3", "out", "cout_total", "cout_off", "s"]
    for decl, ct in zip(args, sig):
        want = "pointer" if "*" in decl or decl.startswith("gp_stream_t") else "int"
        assert want == ("int" if ct is ctypes.c_int else "pointer"), (decl, ct)
    assert "sa_lds_bf16x9.hip" in build.SOURCES
    build.build()
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), "gp_sa_lds_bf16x9")
    assert prototype("gp_sa_pre_mlp_max_bf16x9")  # the level-2 entry point keeps its own name


def test_config_field_resolves_by_sampler():
    from genpose_amd.config import encoder_level1_of, encoder_level3_of, encoder_precision_of, get_config
    assert get_config().encoder_level1 == "auto"
    assert encoder_level1_of(get_config(sampler_mode=["pc"])) == "bf16x9"
    for mode, steps in ((["ode"], None), (["heun"], 8), (["dpm2m"], 8)):
        assert encoder_level1_of(get_config(sampler_mode=mode, sampling_steps=steps)) == "f32mfma"
    assert encoder_level1_of(get_config(sampler_mode=["ode"], encoder_level1="bf16x9")) == "bf16x9"   # the opt-in
    assert encoder_level1_of(get_config(sampler_mode=["pc"], encoder_level1="f32mfma")) == "f32mfma"  # the opt-out
    # the other levels' fields are independent, and encoder_precision_of's mapping is what it was
    cfg = get_config(sampler_mode=["pc"], encoder_level1="f32mfma")
    assert encoder_precision_of(cfg) == "bf16x9" and encoder_level3_of(cfg) == "bf16x9"
    assert encoder_precision_of(get_config(sampler_mode=["ode"], encoder_level1="bf16x9")) == "f32"
    with pytest.raises(ValueError):
        encoder_level1_of(get_config(encoder_level1="fp8"))

    class Bare:  # the reference's own namespace has no such field: 'auto'
        sampler_mode = ["pc"]
    assert encoder_level1_of(Bare()) == "bf16x9"
