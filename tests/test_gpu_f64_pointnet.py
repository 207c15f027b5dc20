"""GPU: the vanilla PointNet kernels (csrc/pointnet.hip: gp_pointnet_stn_pool, gp_pointnet_feat_pool, gp_dense_rows) against FLOAT64.

The rule is test_gpu_f64_score.py's: E_oracle = the float32 CPU reference's own error against the float64 reference
(tests/pointnet_reference.py: e_oracle, one value per quantity, maximised over the case set); a device result passes when its error
(max |got - ref| / max |ref|, per cloud) is at most MARGIN x E_oracle.  MARGIN = 3 was fixed before any kernel was measured.

  a  the two pooled kernels through the C ABI, one quantity at a time: stn_pool against g, feat_pool FED THE CPU REFERENCE'S trans
     (a wrong x . trans cannot hide behind the device's own trans); sign pattern; no channel above the float64 maximum (a padding row
     or a neighbouring cloud's row that leaks into the maximum can only raise it)
  b  the whole encoder, trans and feat separately; capture and replay equal the direct pass bit for bit
  c  gp_dense_rows directly: one to four row tiles, ragged channel groups, a second k iteration, both halves; guard floats around the
     output, NaN guard rows behind every input; integer inputs, on which the result must EQUAL the float64 one
  d  the integer network (weights in {-1, 0, 1}): both pooled kernels and the encoder equal the reference bit for bit
  e  a cloud's features do not depend on the order of its points, on appended duplicates, on its place in the batch, or on a NaN / Inf in
     another cloud - bit for bit
  f  the pointnet_and_pointnet2 agent's fused feature on the fixture's three 1024-point clouds
  g  positive control: trunk weights with their low 8 mantissa bits cleared FAIL the rule on every weight set

Case set: weights seed0 / seed1 / stress x shapes (1,1) (2,47) (2,48) (3,49) (2,96) (2,97) (17,49) (9,145) x clouds randn * 0.1 + {0, 0.5}
(the tile is 48 points; 17 clouds are three row tiles of gp_dense_rows).  Every ratio is printed (pytest -s); profiles/f64_pointnet.txt
keeps a run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import f64_reference as fr
import pointnet_reference as pr
from genpose_amd import _lib
from genpose_amd._lib import ptr, stream_ptr

INDEPENDENCE_SHAPES = ((3, 49), (2, 97), (9, 145))
SENTINEL, GUARD = -7.25, 64


@pytest.fixture(scope="module")
def enc_of():
    from genpose_amd.pointnet_encoder import PointNetEncoderHIP
    cache = {}

    def get(which):
        if which not in cache:
            sd = pr.integer_state_dict() if which == "integer" else pr.state_dict(which)
            cache[which] = PointNetEncoderHIP(sd, "cuda", prefix=pr.PN)
        return cache[which]
    return get


def dev_stn_pool(w, pts):
    B, n, _ = pts.shape
    g = torch.empty(B, 1024, device="cuda")
    _lib.call("gp_pointnet_stn_pool", B, n, ptr(pts), *[ptr(t) for pair in w.stn_convs for t in pair], ptr(g), stream_ptr())
    return g


def dev_feat_pool(w, pts, trans):
    B, n, _ = pts.shape
    feat = torch.empty(B, 1024, device="cuda")
    _lib.call("gp_pointnet_feat_pool", B, n, ptr(pts), ptr(trans), *[ptr(t) for pair in w.convs for t in pair], ptr(feat), stream_ptr())
    return feat


def _gate(what, which, where, eo, ed, bad, margin=fr.MARGIN):
    print(f"pnf64 | {what:16s} | {which:7s} | {where:18s} | oracle {eo:.2e} | device {ed:.2e} | ratio {ed / eo:6.3f}")
    assert 0 < eo < fr.ORACLE_CEILING
    if not ed <= margin * eo:
        bad.append((what, which, where, eo, ed, round(ed / eo, 3)))


def _pooled(what, which, where, got, ref64, eo, bad):
    """the rule, the sign pattern and `no channel above the float64 maximum` of one pooled quantity [B,1024]"""
    got = got.double().cpu()
    _gate(what, which, where, eo, pr.cloud_error(got, ref64), bad)
    big = ref64.abs() > 1e-3
    if not torch.equal(torch.sign(got[big]), torch.sign(ref64[big])):
        bad.append((what, which, where, "sign pattern"))
    over = got - ref64 - fr.MARGIN * eo * ref64.abs().max(dim=1, keepdim=True)[0]
    if not bool((over <= 0).all()):
        bad.append((what, which, where, "above the float64 maximum", int((over > 0).sum()), float(over.max())))


# ----------------------------------------------------------------------------- a, b
@pytest.mark.parametrize("which", pr.WEIGHTS)
def test_pooled_kernels_one_quantity_at_a_time(enc_of, which):
    w = enc_of(which).w
    bad = []
    for B, n in pr.SHAPES:
        for off in pr.OFFSETS:
            c, where = pr.case(which, B, n, off), f"({B},{n}) off {off}"
            pts = c["pts"].cuda()
            _pooled("stn_pool", which, where, dev_stn_pool(w, pts), c["g64"], pr.e_oracle("g"), bad)
            _pooled("feat_pool|trans", which, where, dev_feat_pool(w, pts, c["trans32"].contiguous().cuda()), c["feat_gt64"],
                    pr.e_oracle("feat_given_trans"), bad)
    assert not bad, bad


@pytest.mark.parametrize("which", pr.WEIGHTS)
def test_whole_encoder(enc_of, which):
    enc = enc_of(which)
    bad = []
    for B, n in pr.SHAPES:
        for off in pr.OFFSETS:
            c, where = pr.case(which, B, n, off), f"({B},{n}) off {off}"
            feat, trans = enc.forward(c["pts"].cuda(), return_trans=True)
            _gate("trans", which, where, pr.e_oracle("trans"), pr.cloud_error(trans.double().cpu(), c["trans64"]), bad)
            _pooled("feat", which, where, feat, c["feat64"], pr.e_oracle("feat"), bad)
    assert not bad, bad


@pytest.mark.parametrize("B,n", [(3, 49), (17, 49)])
def test_replay_is_the_direct_pass(enc_of, B, n):
    enc = enc_of("seed0")
    pts = pr.clouds(B, n, 0.5).cuda()
    direct = enc.forward(pts)
    runs = [enc.encode(pts) for _ in range(3)]  # launch by launch, captures, replays
    assert (B, n, 3) in enc._pass_graphs
    for r in runs:
        assert torch.equal(r, direct)


# ----------------------------------------------------------------------------- c
def _guarded(t, rows_after=3):
    """a device copy of the 2-D tensor with `rows_after` rows of NaN behind it: a load past the end shows in the result"""
    buf = torch.full((t.shape[0] + rows_after, t.shape[1]), float("nan"), device="cuda")
    buf[:t.shape[0]] = t.cuda()
    return buf, buf[:t.shape[0]]


def _dense_on_device(i, integer):
    """case i through gp_dense_rows -> out [rows, n_out] on the host; asserts the guards around the output and behind the inputs"""
    rows, ka, kb, n_out, act = pr.DENSE_CASES[i]
    xa, xb, W, b = pr.dense_inputs(i, integer)
    bufs = [_guarded(t) for t in (xa, W, b[None, :])] + ([_guarded(xb)] if kb else [])
    views = [v for _, v in bufs]
    out_buf = torch.full((GUARD + rows * n_out + GUARD,), SENTINEL, device="cuda")
    out = out_buf[GUARD:GUARD + rows * n_out]
    _lib.call("gp_dense_rows", rows, ka, kb, n_out, ptr(views[0]), ptr(views[3]) if kb else None, ptr(views[1]), ptr(views[2]), act, ptr(out),
              stream_ptr())
    torch.cuda.synchronize()
    assert bool((out_buf[:GUARD] == SENTINEL).all()) and bool((out_buf[GUARD + rows * n_out:] == SENTINEL).all()), pr.DENSE_CASES[i]
    for (buf, v), t in zip(bufs, (xa, W, b[None, :], xb)):
        assert torch.equal(v.cpu(), t) and bool(torch.isnan(buf[t.shape[0]:]).all())
    return out.view(rows, n_out).cpu()


def test_dense_rows_against_float64():
    bad = []
    eo = pr.e_oracle("dense")
    for i, case in enumerate(pr.DENSE_CASES):
        out = _dense_on_device(i, integer=False)
        assert bool(torch.isfinite(out).all()), case
        _gate("dense_rows", "randn", str(case), eo, fr.block_error(out, pr.dense_reference(i, torch.float64), None)[0], bad)
    assert not bad, bad


def test_dense_rows_on_integers_is_exact():
    """integer inputs, weights and biases in [-4, 4]: every partial sum is exact in fp32 in any order, so an indexing error cannot pass
    as rounding - at K = 4 and K = 8, where MARGIN x E_oracle is loose, too"""
    for i, case in enumerate(pr.DENSE_CASES):
        out, ref = _dense_on_device(i, integer=True), pr.dense_reference(i, torch.float64, integer=True)
        assert torch.equal(out.double(), ref), (case, int((out.double() != ref).sum()))


# ----------------------------------------------------------------------------- d
@pytest.mark.parametrize("B,n", pr.INTEGER_SHAPES)
def test_integer_network_bit_for_bit(enc_of, B, n):
    enc = enc_of("integer")
    sd64 = fr.f64_state_dict(pr.integer_state_dict())
    pts = pr.integer_clouds(B, n)
    eye = torch.eye(3).expand(B, 3, 3).contiguous()
    g = dev_stn_pool(enc.w, pts.cuda()).double().cpu()
    assert torch.equal(g, pr.stn_pool(sd64, pts)), int((g != pr.stn_pool(sd64, pts)).sum())
    f = dev_feat_pool(enc.w, pts.cuda(), eye.cuda()).double().cpu()
    ref = pr.feat_pool(sd64, pts, eye)
    assert torch.equal(f, ref), int((f != ref).sum())
    feat, trans = enc.forward(pts.cuda(), return_trans=True)
    assert torch.equal(trans.cpu(), eye) and torch.equal(feat.double().cpu(), ref)


# ----------------------------------------------------------------------------- e
def _same(enc, pts, feat, trans, rows, what):
    f, t = enc.forward(pts.cuda().contiguous(), return_trans=True)
    assert torch.equal(f[rows], feat) and torch.equal(t[rows], trans), what


@pytest.mark.parametrize("which", ["seed0", "stress"])
@pytest.mark.parametrize("B,n", INDEPENDENCE_SHAPES)
def test_features_depend_on_the_cloud_as_a_set_only(enc_of, which, B, n):
    enc = enc_of(which)
    pts = pr.clouds(B, n, 0.5)
    g = torch.Generator().manual_seed(4000 + B + n)
    feat, trans = enc.forward(pts.cuda(), return_trans=True)
    everything = slice(None)
    # the order of a cloud's points
    perm = torch.stack([pts[b, torch.randperm(n, generator=g)] for b in range(B)])
    assert not torch.equal(perm, pts) or n == 1
    _same(enc, perm, feat, trans, everything, "permutation")
    # appended copies of points the cloud already has: every tile boundary moves
    for k in (1, 47, 48):
        idx = torch.randint(0, n, (B, k), generator=g)
        more = torch.cat([pts, torch.stack([pts[b, idx[b]] for b in range(B)])], dim=1)
        _same(enc, more, feat, trans, everything, f"{k} duplicates")
    for i in sorted({0, B // 2, B - 1}):
        others = torch.cat([pts[:i], pts[i + 1:]])
        # alone, first and last in the batch
        _same(enc, pts[i:i + 1], feat[i:i + 1], trans[i:i + 1], everything, f"cloud {i} alone")
        _same(enc, torch.cat([pts[i:i + 1], others]), feat[i], trans[i], 0, f"cloud {i} first")
        _same(enc, torch.cat([others, pts[i:i + 1]]), feat[i], trans[i], B - 1, f"cloud {i} last")
        # a NaN / an Inf coordinate in every other cloud
        for bad_value in (float("nan"), float("inf")):
            spoiled = pts.clone()
            for b in range(B):
                if b != i:
                    spoiled[b, int(torch.randint(0, n, (1,), generator=g)), int(torch.randint(0, 3, (1,), generator=g))] = bad_value
            _same(enc, spoiled, feat[i], trans[i], i, f"cloud {i} beside {bad_value}")


# ----------------------------------------------------------------------------- f
def test_fused_feature_against_float64():
    from test_gpu_pointnet import fused_agent
    bad = []
    for mode in ("score", "energy"):
        c = pr.fused_case(mode)
        agent = fused_agent(mode, sd=pr.state_dict("seed0", mode))
        feat = agent.net({"pts": c["pts"].cuda()}, mode="pts_feature").double().cpu()
        _gate("fused feature", "seed0", f"{mode} (3,1024)", pr.e_oracle("fused"), pr.cloud_error(feat, c["f64"]), bad)
    assert not bad, bad


# ----------------------------------------------------------------------------- g
def test_rule_rejects_weights_without_their_low_8_bits():
    """positive control: the trunk's four weight matrices with the low 8 of their 24 mantissa bits cleared on the host before packing
    (a relative change of up to 2^-15 per weight) must FAIL the rule on every weight set"""
    from genpose_amd.weights import PointNetWeights
    eo = pr.e_oracle("feat_given_trans")
    for which in pr.WEIGHTS:
        sd = dict(pr.state_dict(which))
        for name in ("conv1", "conv2", "conv3", "conv4"):
            W = sd[pr.PN + name + ".weight"]
            sd[pr.PN + name + ".weight"] = (W.contiguous().view(torch.int32) & ~0xFF).view(torch.float32)
        w = PointNetWeights(sd, "cuda", prefix=pr.PN)
        worst = 0.0
        for B, n in ((3, 49), (9, 145)):
            c = pr.case(which, B, n, 0.5)
            got = dev_feat_pool(w, c["pts"].cuda(), c["trans32"].contiguous().cuda()).double().cpu()
            worst = max(worst, pr.cloud_error(got, c["feat_gt64"]))
        print(f"pnf64 | control: 8 bits off  | {which:7s} | oracle {eo:.2e} | device {worst:.2e} | ratio {worst / eo:6.3f}")
        assert worst > fr.MARGIN * eo, (which, worst / eo)
