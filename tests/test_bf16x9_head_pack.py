"""Host side of the chunk-major heads of the exact-product split-bf16 trunk (csrc/trunk_bf16x9.h): the head pack in the order the ring
consumes it, [head 3][chunk pair 8][chunk 2][k-block 8][term 3][64][8], against a slow per-element gather from split_bf16x9; it is a
permutation of pack_bf16x9(W, 48, 8)."""
import torch


def _slow_head_pack(terms):
    """out[h][j][c][kb][t][lane][e] = term t of W[256 h + 16 (2 j + c) + n][32 kb + koff(g, e)], lane = (n = lane % 16, g = lane // 16),
    koff = 4 g + e (e < 4) or 16 + 4 g + e - 4: the register chain's k order."""
    out = torch.zeros(3, 8, 2, 8, len(terms), 64, 8, dtype=torch.int16)
    for h in range(3):
        for j in range(8):
            for c in range(2):
                for kb in range(8):
                    for lane in range(64):
                        n, g = lane % 16, lane // 16
                        for e in range(8):
                            koff = 4 * g + e if e < 4 else 16 + 4 * g + e - 4
                            for t, term in enumerate(terms):
                                out[h, j, c, kb, t, lane, e] = term[256 * h + 16 * (2 * j + c) + n, 32 * kb + koff]
    return out


def test_head_pack_matches_the_per_element_definition():
    from genpose_amd.weights import pack_bf16x9, pack_heads_bf16x9, split_bf16x9
    W = torch.randn(768, 256, generator=torch.Generator().manual_seed(11))
    p = pack_heads_bf16x9(W)
    assert p.shape == (3, 8, 2, 8, 3, 64, 8) and p.dtype == torch.int16 and p.is_contiguous()
    assert torch.equal(p, _slow_head_pack([t.view(torch.int16) for t in split_bf16x9(W)]))
    # a permutation of the k-major pack: slice (h, j) holds chunks 16 h + 2 j, + 1 of every k-block
    k_major = pack_bf16x9(W, 48, 8)
    for h in range(3):
        for j in range(8):
            for c in range(2):
                assert torch.equal(p[h, j, c], k_major[:, 16 * h + 2 * j + c])


def test_head_pack_refuses_other_shapes():
    import pytest
    from genpose_amd.weights import pack_heads_bf16x9
    with pytest.raises(ValueError):
        pack_heads_bf16x9(torch.randn(768, 128))
