"""GPU parity at cloud sizes other than 1024 points: the entry points the encoder launches for its grouping (gp_fps_chain[_arith],
gp_ball_query_msg[_arith]) against the C oracle at the sizes where their control flow changes, and the whole encoder against
oracle.genpose_oracle.encoder_forward from 600 to 6000 points per cloud.  Index outputs are compared bit for bit; every output is
allocated with a sentinel tail that must come back untouched."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import genpose_oracle as go
from oracle import pn2_oracle as ops

# the project's encoder bound (tests/test_gpu_encoder.py ENC_RTOL / ENC_ATOL: fp32 MFMA chain against oneDNN conv + separate BN on O(1)
# features); the bf16x9 level-2 kernel is held to the same one - its recorded error against float64 is the fp32 kernel's class
# (profiles/r10_sa_bf16x9.txt)
ENC_RTOL, ENC_ATOL = 2e-4, 2e-4
TAIL = 64  # sentinel elements behind every output: -7 (indices) / NaN (coordinates)


@pytest.fixture(params=["A", "B", "C"])
def arith(request):
    """Every contraction convention of the squared distances (include/genpose_hip.h GP_ARITH_*): the oracle is switched, and the
    `_arith` entry points get the same convention's code."""
    with ops.use_arith(request.param):
        yield request.param


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tailed(shape, fill, dtype):
    """(whole buffer, view of `shape` at its start): the view is what the kernel is given, the TAIL elements behind it must survive."""
    n = int(np.prod(shape))
    flat = torch.full((n + TAIL,), fill, dtype=dtype, device="cuda")
    return flat, flat[:n].view(shape)


def untouched(t, fill):
    t = t.cpu()
    return bool(torch.isnan(t).all()) if fill != fill else bool((t == fill).all())


def tail_intact(buf, fill):
    flat, view = buf
    return untouched(flat[view.numel():], fill)


NAN = float("nan")


# ---------------------------------------------------------------------------------------------- 1. gp_fps_chain
def chain_clouds(n0):
    """As test_gpu_ops.test_fps_vs_oracle: a random cloud, one snapped to a 1/50 grid (exact ties), one whose second half repeats its
    first (exact duplicates)."""
    rng = np.random.default_rng(n0 * 7 + 1)
    xyz = (rng.normal(size=(3, n0, 3)) * 0.1).astype(np.float32)
    xyz[1] = np.round(xyz[1] * 50) / 50
    if n0 > 8:
        xyz[2, n0 // 2:] = xyz[2, : n0 - n0 // 2]
    return xyz


def fps_chain(entry, ac, xyz, ms, n0=None, nlevels=None, m_arg=None):
    """One launch of `entry` over freshly allocated, sentinel-filled outputs: (return code, index buffers, coordinate buffers)."""
    from genpose_amd import _lib
    from genpose_amd._lib import ptr, stream_ptr
    B = xyz.shape[0]
    x = dev(xyz)
    bi = [tailed((B, m), -7, torch.int32) for m in ms]
    bx = [tailed((B, m, 3), NAN, torch.float32) for m in ms]
    pi = [ptr(bi[l][1]) if l < len(ms) else None for l in range(3)]
    px = [ptr(bx[l][1]) if l < len(ms) else None for l in range(3)]
    m_arg = list(ms if m_arg is None else m_arg)
    marr = (ctypes.c_int * 4)(*(m_arg + [0] * (4 - len(m_arg))))
    args = [B, xyz.shape[1] if n0 is None else n0, len(ms) if nlevels is None else nlevels, marr, ptr(x), pi[0], px[0], pi[1], px[1], pi[2],
            px[2], stream_ptr()]
    if entry.endswith("_arith"):
        args.insert(0, ac)
    rc = getattr(_lib.lib(), entry)(*args)
    torch.cuda.synchronize()
    return rc, bi, bx


def oracle_chain(xyz, ms):
    """The chain level by level on the host: FPS of the previous level's gathered coordinates, then the gather."""
    cur, out = xyz, []
    for m in ms:
        idx, _ = ops.furthest_point_sampling(cur, m)
        new = ops.gather_points(np.ascontiguousarray(cur.transpose(0, 2, 1)), idx).transpose(0, 2, 1)
        cur = np.ascontiguousarray(new)
        out.append((idx, cur))
    return out


# (n0, m per level): every arm of fps_level's dispatch (points per lane 16 .. 1, with and without bounds checks), a rank with a quotient
# (n no power of two), planes whose capacity is not the level's size, the 64-pick flush at m = 1 / 64 / 65, one and two levels
CHAIN_SHAPES = [
    (1000, [400, 200, 100]),  # 16, 8, 4 points per lane, all with bounds checks
    (1023, [512, 256, 128]),  # a bounds-checked level, then the exact-size levels behind it
    (300, [150, 70, 33]),     # 8, 4, 2 points per lane, bounds-checked
    (130, [129, 65, 64]),     # m = n - 1, m = 65, m = 64
    (64, [64, 64, 64]),       # every point selected; one point per lane, exact size
    (40, [20, 10]),           # one point per lane with bounds checks; two levels, third pointers null
    (700, [1]),               # one level, m = 1
    (3, [2, 1]),              # smallest chain of two levels
    (1, [1]),                 # single point
]


@pytest.mark.parametrize("n0,ms", CHAIN_SHAPES, ids=[f"{n}-{'-'.join(map(str, m))}" for n, m in CHAIN_SHAPES])
def test_fps_chain_vs_oracle(arith, n0, ms):
    from genpose_amd.config import dist_arith_code
    xyz = chain_clouds(n0)
    rc, bi, bx = fps_chain("gp_fps_chain_arith", dist_arith_code(arith), xyz, ms)
    assert rc == 0
    for l, (idx, new) in enumerate(oracle_chain(xyz, ms)):
        assert np.array_equal(bi[l][1].cpu().numpy(), idx), f"level {l}: indices"
        assert np.array_equal(bx[l][1].cpu().numpy(), new), f"level {l}: gathered coordinates"
        assert tail_intact(bi[l], -7) and tail_intact(bx[l], NAN), f"level {l}: wrote past its output"


def test_fps_chain_default_entry_is_convention_b():
    from genpose_amd import _lib
    from genpose_amd.config import dist_arith_code
    assert _lib.lib().gp_arith_default() == dist_arith_code("B")
    xyz = chain_clouds(300)
    rc_d, bi_d, bx_d = fps_chain("gp_fps_chain", None, xyz, [150, 70, 33])
    rc_b, bi_b, bx_b = fps_chain("gp_fps_chain_arith", dist_arith_code("B"), xyz, [150, 70, 33])
    assert rc_d == rc_b == 0
    for l in range(3):
        assert torch.equal(bi_d[l][1], bi_b[l][1]) and torch.equal(bx_d[l][1], bx_b[l][1])
        assert tail_intact(bi_d[l], -7) and tail_intact(bx_d[l], NAN)
    with ops.use_arith("B"):
        assert np.array_equal(bi_d[2][1].cpu().numpy(), oracle_chain(xyz, [150, 70, 33])[2][0])


@pytest.mark.parametrize("entry", ["gp_fps_chain_arith", "gp_fps_chain"])
def test_fps_chain_argument_contract(entry):
    """A level larger than the one before it, more than 1024 points, four levels: -1 (GP_EINVAL) before any launch - nothing is written."""
    from genpose_amd.config import dist_arith_code
    ac = dist_arith_code("B")
    cases = [
        dict(xyz=chain_clouds(100)[:2], ms=[50, 60]),                                   # m[1] > m[0]
        dict(xyz=chain_clouds(100)[:2], ms=[101]),                                      # m[0] > n0
        dict(xyz=chain_clouds(1025)[:1], ms=[512]),                                     # n0 > 1024
        dict(xyz=chain_clouds(100)[:2], ms=[50, 40, 30], nlevels=4, m_arg=[50, 40, 30, 20]),  # nlevels = 4
    ]
    for c in cases:
        rc, bi, bx = fps_chain(entry, ac, **c)
        assert rc == -1, c["ms"]
        for l in range(len(c["ms"])):
            assert untouched(bi[l][0], -7) and untouched(bx[l][0], NAN), (c["ms"], l)


# ---------------------------------------------------------------------------------------------- 2. gp_ball_query_msg
def ball_query_msg(entry, ac, xyz, new, r0, ns0, r1, ns1):
    """One launch over outputs prefilled with -7 (the entry zero-fills empty rows itself): (return code, buffer of scale 0, of scale 1)."""
    from genpose_amd import _lib
    from genpose_amd._lib import ptr, stream_ptr
    B, n, _ = xyz.shape
    m = new.shape[1]
    b0 = tailed((B, m, ns0), -7, torch.int32)
    b1 = tailed((B, m, ns1), -7, torch.int32)
    x, c = dev(xyz), dev(new)
    args = [B, n, m, r0, ns0, r1, ns1, ptr(c), ptr(x), ptr(b0[1]), ptr(b1[1]), stream_ptr()]
    if entry.endswith("_arith"):
        args.insert(0, ac)
    rc = getattr(_lib.lib(), entry)(*args)
    torch.cuda.synchronize()
    return rc, b0, b1


def msg_clouds(n, m):
    """As test_gpu_ops.test_ball_query_vs_oracle: centres are a random subset of the cloud; centre 0 is moved away from every point."""
    rng = np.random.default_rng(n + m)
    xyz = (rng.normal(size=(2, n, 3)) * 0.08).astype(np.float32)
    new = np.ascontiguousarray(xyz[:, rng.permutation(n)[:m]])
    new[:, 0] += 100.0
    return xyz, new


MSG_SHAPES = [
    (700, 50, 0.05, 16, 0.1, 32),      # n % 64 != 0 (bounds-checked scan), m % 16 != 0 (partial last workgroup)
    (70, 3, 0.05, 8, 10.0, 64),        # n % 4 != 0 (scalar staging); the second radius takes the whole cloud
    (1023, 512, 0.02, 16, 0.04, 32),   # large odd n
    (1500, 300, 0.04, 5, 0.08, 70),    # nsample a multiple of nothing, and more than 64 (second round of the row store)
    (5053, 33, 0.1, 16, 0.2, 32),      # the largest n the fused kernel takes
    (64, 17, 1e-6, 16, 1e-6, 32),      # only the centre itself hits
]


@pytest.mark.parametrize("n,m,r0,ns0,r1,ns1", MSG_SHAPES, ids=[f"n{s[0]}-m{s[1]}-ns{s[3]}-{s[5]}" for s in MSG_SHAPES])
def test_ball_query_msg_vs_oracle(arith, n, m, r0, ns0, r1, ns1):
    from genpose_amd import _lib
    from genpose_amd.config import dist_arith_code
    assert _lib.lib().gp_ball_query_msg_fits(n, ns0, ns1) == 1
    xyz, new = msg_clouds(n, m)
    rc, b0, b1 = ball_query_msg("gp_ball_query_msg_arith", dist_arith_code(arith), xyz, new, r0, ns0, r1, ns1)
    assert rc == 0
    for buf, r, ns in ((b0, r0, ns0), (b1, r1, ns1)):
        got = buf[1].cpu().numpy()
        assert np.array_equal(got, ops.ball_query(r, ns, xyz, new)), f"radius {r}, {ns} samples"
        assert np.all(got[:, 0] == 0), "a centre without a neighbour: zero row, whatever the buffer held"
        assert tail_intact(buf, -7)
    if r0 == 1e-6:  # the centres are points of the cloud: each finds itself and nothing else
        got = b1[1].cpu().numpy()[:, 1:]
        assert all(len(set(row)) == 1 for row in got.reshape(-1, ns1))


@pytest.mark.parametrize("entry", ["gp_ball_query_msg_arith", "gp_ball_query_msg"])
def test_ball_query_msg_radius_tie_is_strict(entry):
    """As test_gpu_ops.test_ball_query_radius_tie_is_strict, through the fused entry: d2 < r^2 is strict in both scales (points at exactly
    0.5 from the centre with r0 = 0.5, at exactly 0.25 with r1 = 0.25)."""
    from genpose_amd.config import dist_arith_code
    xyz = np.array([[[0, 0, 0], [0.5, 0, 0], [0.25, 0, 0], [0, 0.5, 0]]], dtype=np.float32)
    new = np.array([[[0, 0, 0]]], dtype=np.float32)
    rc, b0, b1 = ball_query_msg(entry, dist_arith_code("B"), xyz, new, 0.5, 4, 0.25, 4)
    assert rc == 0
    assert b0[1].cpu().numpy().tolist() == ops.ball_query(0.5, 4, xyz, new).tolist() == [[[0, 2, 0, 0]]]
    assert b1[1].cpu().numpy().tolist() == ops.ball_query(0.25, 4, xyz, new).tolist() == [[[0, 0, 0, 0]]]
    assert tail_intact(b0, -7) and tail_intact(b1, -7)


@pytest.mark.parametrize("entry", ["gp_ball_query_msg_arith", "gp_ball_query_msg"])
def test_ball_query_msg_refuses_what_does_not_fit(entry):
    """include/genpose_hip.h: a cloud that does not fit the fused kernel's LDS (n = 5054 at 16 + 32 samples) is refused with -1 (GP_EINVAL)
    before any launch and nothing is written; gp_ball_query_msg_fits is where a caller asks."""
    from genpose_amd import _lib
    from genpose_amd.config import dist_arith_code
    fits = _lib.lib().gp_ball_query_msg_fits
    assert fits(5053, 16, 32) == 1 and fits(5054, 16, 32) == 0
    xyz, new = msg_clouds(5054, 33)
    rc, b0, b1 = ball_query_msg(entry, dist_arith_code("B"), xyz, new, 0.1, 16, 0.2, 32)
    assert rc == -1
    assert untouched(b0[0], -7) and untouched(b1[0], -7)


# ---------------------------------------------------------------------------------------------- 3. the encoder
ENC_SIZES = [600, 700, 1023, 1500, 2048, 4096, 5053, 5054, 6000]


@pytest.fixture(scope="module")
def sd():
    return go.make_state_dict(0, "score")


@pytest.fixture(scope="module")
def encoders(sd):
    """One encoder per precision for the whole module (their workspaces are keyed by batch and size)."""
    from genpose_amd.encoder import Pointnet2EncoderHIP
    return {p: Pointnet2EncoderHIP(sd, "cuda", precision=p) for p in ("f32", "bf16x9")}


@functools.lru_cache(maxsize=None)
def clouds(N, tiled=False):
    from genpose_amd import synth
    if not tiled:
        return synth.make_batch(2, start=11, n_pts=N)
    pts = synth.make_batch(3, start=11, n_pts=N)
    pts[2] = np.tile(pts[2, :64], (N // 64 + 1, 1))[:N]  # 64 distinct points: every distance tied many times over
    return pts


@functools.lru_cache(maxsize=None)
def oracle_encoder(N, tiled=False, params="light"):
    """(features [B,1024], per-level records) of the host oracle, computed once per input and shared by the tests below."""
    from genpose_amd.weights import ENCODER_CFGS
    sd = go.make_state_dict(0, "score", params)
    ref, inter = go.encoder_forward(sd, torch.from_numpy(clouds(N, tiled)), cfg=ENCODER_CFGS[params], return_intermediates=True)
    return ref.numpy(), inter


def check_against_oracle(enc, pts_np, ref, inter, what):
    feat, ws = enc.forward(torch.from_numpy(pts_np).cuda(), return_intermediates=True)
    cfg = enc.cfg
    for lvl, npnt in enumerate(cfg["npoints"]):
        if npnt is None:
            break
        assert np.array_equal(ws["fps_idx"][lvl].cpu().numpy(), inter[lvl]["fps_idx"]), f"{what}: FPS level {lvl}"
        assert np.array_equal(ws["new_xyz"][lvl].cpu().numpy(), inter[lvl]["new_xyz"]), f"{what}: centres level {lvl}"
        for s in range(len(cfg["radii"][lvl])):
            assert np.array_equal(ws["bq"][lvl][s].cpu().numpy(), inter[lvl][f"bq_idx{s}"]), f"{what}: ball query level {lvl} scale {s}"
    got = feat.cpu().numpy()
    print(f"{what}: max |feat - oracle| = {np.abs(got - ref).max():.3e} (|oracle| max {np.abs(ref).max():.3f})")
    np.testing.assert_allclose(got, ref, rtol=ENC_RTOL, atol=ENC_ATOL, err_msg=what)
    return feat


@pytest.mark.parametrize("N", ENC_SIZES)
def test_encoder_f32_at_other_sizes(encoders, N):
    """600 .. 1023: the chain kernel at an n0 that is no power of two; 1025 .. 2048 / .. 4096 / beyond: the three wide FPS kernels, one launch
    and one gather per level; 5054 and 6000: level 0's cloud no longer fits the two-scale ball query (one query per scale instead)."""
    check_against_oracle(encoders["f32"], clouds(N), *oracle_encoder(N), f"f32 N={N}")


def test_encoder_f32_tiled_cloud_at_700(encoders):
    check_against_oracle(encoders["f32"], clouds(700, True), *oracle_encoder(700, True), "f32 N=700, last cloud 64 points tiled")


@pytest.mark.parametrize("N", [700, 1500])
def test_encoder_bf16x9_at_other_sizes(encoders, N):
    assert "bf16x9" in encoders["bf16x9"].sa_kernels.values()
    check_against_oracle(encoders["bf16x9"], clouds(N), *oracle_encoder(N), f"bf16x9 N={N}")


@pytest.mark.parametrize("N", [700, 1500])
def test_encode_graph_shared_grouping_and_batch_independence(sd, N):
    """encode() direct / capturing / replaying returns forward()'s bits on whichever grouping sequence N selects; the workspace it
    returns serves an encoder with other weights; a cloud's features do not depend on its batch."""
    from genpose_amd.encoder import Pointnet2EncoderHIP
    enc = Pointnet2EncoderHIP(sd, "cuda")  # its own: the first / second / third call of a shape are direct / capture / replay
    pts = torch.from_numpy(clouds(N)).cuda()
    want = enc.forward(pts).clone()
    np.testing.assert_allclose(want.cpu().numpy(), oracle_encoder(N)[0], rtol=ENC_RTOL, atol=ENC_ATOL)
    for call in ("direct", "capture", "replay"):
        feat, ws = enc.encode(pts)
        assert torch.equal(feat, want), f"encode() {call}"
    assert len(enc._pass_graphs) == 1  # the third call did replay a captured pass
    enc_e = Pointnet2EncoderHIP(go.make_state_dict(0, "energy"), "cuda")
    own = enc_e.forward(pts).clone()
    assert not torch.equal(own, want)
    assert torch.equal(enc_e.forward(pts, grouping=ws), own)
    assert torch.equal(enc.forward(pts[1:2]), want[1:2])


def test_too_few_points_raise_and_leave_the_encoder_usable(sd):
    """300 points: fewer than level 0 selects.  The call raises; the encoder's next pass at 1024 points is the oracle's."""
    from genpose_amd import synth
    from genpose_amd._lib import GenposeHipError
    from genpose_amd.encoder import Pointnet2EncoderHIP
    enc = Pointnet2EncoderHIP(sd, "cuda")
    with pytest.raises((GenposeHipError, ValueError)):
        enc.forward(torch.from_numpy(synth.make_batch(2, start=11, n_pts=300)).cuda())
    torch.cuda.synchronize()
    check_against_oracle(enc, clouds(1024), *oracle_encoder(1024), "f32 N=1024 after a refused N=300")


@pytest.mark.parametrize("params", ["dense", "lighter"])
def test_other_configurations_at_700(params):
    """'dense' at 700 points: neighbourhoods of 32 + 64 and 8 + 16 samples through the chain kernel and the two-scale ball query.  'lighter':
    FOUR grouping levels, which the chain kernel does not take - below 1024 points too it is one FPS launch and one gather per level,
    with single-scale ball queries."""
    from genpose_amd.encoder import Pointnet2EncoderHIP
    enc = Pointnet2EncoderHIP(go.make_state_dict(0, "score", params), "cuda", params)
    assert sum(1 for n in enc.cfg["npoints"] if n is not None) == (4 if params == "lighter" else 3)
    check_against_oracle(enc, clouds(700), *oracle_encoder(700, False, params), f"{params} N=700")
