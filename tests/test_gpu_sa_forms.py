"""GPU: the kernel forms of the hoisted set-abstraction entry point that small batches never reach - the persistent chain / ring kernels
with a full grid and a partial last round (non-split ring form included) and the GroupAll ring with and without tiled clouds behind it -
each as a direct call of gp_sa_pre_mlp_max_layout at a batch size derived from the device's CU count, on random coordinates, random
in-range neighbour indices and random input features.  References: gp_sa_mlp_max on the same inputs (the un-hoisted tile kernel,
independent text) and a float64 host evaluation of the folded layers and the max; rtol = atol = 2e-4, test_gpu_sa_paths.py's bound
for a kernel form against the oracle."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import genpose_oracle as go

TOL = dict(rtol=2e-4, atol=2e-4)


@functools.lru_cache(maxsize=None)
def _weights():
    from genpose_amd.weights import EncoderWeights
    return EncoderWeights(go.make_state_dict(0, "score"), "cuda")


def _host_ref(sc, x):
    """x [B, np, ns, cin + 3] float64 rows in the folded layers' order (features, then xyz): relu MLP, max over the neighbourhood"""
    h = x
    for W, b in sc._folded_plain:
        h = torch.relu(h @ W.double().T + b.double())
    return h.max(dim=2)[0].numpy()


def _run_forms(level, scale, B, xyz, feats, new_xyz, idx):
    """-> (hoisted entry point as dispatched, un-hoisted tile kernel): whole [B, np, cout_total] outputs"""
    from genpose_amd import _lib
    from genpose_amd._lib import ptr, stream_ptr
    ew = _weights()
    scales = ew.levels[level]
    sc = scales[scale]
    (w1, b1), (w2, b2), (w3, b3) = sc.layers
    c1, c2, c3 = sc.couts
    cout_all, off = sum(s.couts[2] for s in scales), sum(s.couts[2] for s in scales[:scale])
    n = xyz.shape[1]
    npnt, ns = (1, n) if idx is None else (idx.shape[1], idx.shape[2])
    cin = 0 if feats is None else feats.shape[2]
    st = stream_ptr()
    xd = xyz.cuda()
    fd = None if feats is None else feats.cuda()
    nd = None if new_xyz is None else new_xyz.cuda()
    idd = None if idx is None else idx.cuda()
    z, zstride, zoff = None, 0, 0
    if cin:
        zstride, zoff = sum(s.couts[0] for s in scales), sum(s.couts[0] for s in scales[:scale])
        z = torch.empty(B, n, zstride, device="cuda")
        _lib.call("gp_point_linear", B * n, cin, zstride, ptr(fd), ptr(ew.z_weights[level]), ptr(z), st)
    out_h = torch.zeros(B, npnt, cout_all, device="cuda")
    _lib.call("gp_sa_pre_mlp_max_layout", sc.hidden_layout, B, n, npnt, ns, c1, c2, c3, ptr(xd), ptr(nd), ptr(idd), ptr(z), zstride, zoff,
              ptr(sc.wxyz), ptr(b1), ptr(w2), ptr(b2), ptr(w3), ptr(b3), ptr(out_h), cout_all, off, st)
    out_t = torch.zeros(B, npnt, cout_all, device="cuda")
    _lib.call("gp_sa_mlp_max", B, n, npnt, ns, cin, c1, c2, c3, ptr(xd), ptr(fd), ptr(nd), ptr(idd), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(w3),
              ptr(b3), ptr(out_t), cout_all, off, st)
    torch.cuda.synchronize()
    return out_h.cpu().numpy(), out_t.cpu().numpy(), off, c3


def _check(got_h, got_t, ref, off, c3):
    h, t = got_h[:, :, off:off + c3], got_t[:, :, off:off + c3]
    print(f"max |hoisted - f64| {np.abs(h - ref).max():.3e}  max |tile - f64| {np.abs(t - ref).max():.3e}  max |ref| {np.abs(ref).max():.3e}")
    np.testing.assert_allclose(h, ref, **TOL)
    np.testing.assert_allclose(t, ref, **TOL)
    np.testing.assert_allclose(h, t, **TOL)
    assert np.all(got_h[:, :, :off] == 0) and np.all(got_h[:, :, off + c3:] == 0)  # writes only its slice


@pytest.mark.parametrize("level,scale", [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)])
def test_grouping_level_full_grid_partial_last_round(level, scale):
    """B = CUs / 16 + 1 clouds (17 on 256 CUs): 512 / 256 / 128 B centres against 32 / at most 12 / 8 resident waves per CU on levels 0 /
    1 / 2 - more than one round of every persistent grid, fewer than two, and past the small-batch split of the level-2 ring."""
    cfg = go.LIGHT_CFG
    B = torch.cuda.get_device_properties(0).multi_processor_count // 16 + 1
    n = 1024 if level == 0 else cfg["npoints"][level - 1]
    npnt, ns = cfg["npoints"][level], cfg["nsamples"][level][scale]
    cin = 0 if level == 0 else sum(m[-1] for m in cfg["mlps"][level - 1])
    gen = torch.Generator().manual_seed(100 * level + scale)
    xyz = torch.rand(B, n, 3, generator=gen) * 0.2
    new_xyz = torch.rand(B, npnt, 3, generator=gen) * 0.2
    idx = torch.randint(0, n, (B, npnt, ns), generator=gen, dtype=torch.int32)
    feats = torch.rand(B, n, cin, generator=gen) if cin else None  # (the range of the post-ReLU activations a level reads)
    got_h, got_t, off, c3 = _run_forms(level, scale, B, xyz, feats, new_xyz, idx)
    ar = torch.arange(B)[:, None, None]
    li = idx.long()
    rows = (xyz[ar, li] - new_xyz[:, :, None, :]).double()
    if cin:
        rows = torch.cat([feats[ar, li].double(), rows], dim=-1)
    _check(got_h, got_t, _host_ref(_weights().levels[level][scale], rows), off, c3)


@pytest.mark.parametrize("ring_rounds_plus", ["three_quarters", "one_round_plus_one"])
@pytest.mark.parametrize("scale", [0, 1])
def test_groupall_ring_and_tiles(scale, ring_rounds_plus):
    """GroupAll (c2 = 256 / 384): 3/4 of the CU count = the smallest batch the ring kernel takes whole; CU count + 1 = one ring round and
    one cloud on tiles behind it."""
    cfg = go.LIGHT_CFG
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    B = (3 * ncu) // 4 if ring_rounds_plus == "three_quarters" else ncu + 1
    level = len(cfg["npoints"]) - 1
    assert cfg["npoints"][level] is None
    n, cin = cfg["npoints"][level - 1], sum(m[-1] for m in cfg["mlps"][level - 1])
    gen = torch.Generator().manual_seed(7 + scale)
    xyz = torch.rand(B, n, 3, generator=gen) * 0.2
    feats = torch.rand(B, n, cin, generator=gen)
    got_h, got_t, off, c3 = _run_forms(level, scale, B, xyz, feats, None, None)
    rows = torch.cat([feats.double(), xyz.double()], dim=-1)[:, None]  # [B, 1, n, cin + 3]: absolute coordinates, one neighbourhood
    _check(got_h, got_t, _host_ref(_weights().levels[level][scale], rows), off, c3)
