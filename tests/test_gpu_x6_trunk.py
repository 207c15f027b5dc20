"""GPU: the SIX-product kernels of the PC step's split-bf16 chain plan (csrc/trunk_bf16x9.hip: pc_step_chain_kernel_bf16x6 and its seeded
twin, PCSampler(products=6), config.sampler_products) - lo.lo, lo.mid and mid.lo of every multiply are not issued (csrc/bf16x9.h; the
host-side arithmetic is tests/test_x6_products_host.py).  What a score-model PC agent runs by default on the chain plan.

Held to what the nine-product kernel is held to: the float64 rule of tests/test_gpu_f64_score.py unchanged (MARGIN x the fp32 oracle's own
error, first evaluation at t = 1, the chain plan's shapes, both pose scales, all four weight sets), GATE_VS_F32 x the fp32 chain kernel's
error on the same rows, 30-step runs against the fp32 chain kernel (ragged last workgroup, two batches per launch, gn_ext coupling),
replays, batch independence, PC-100 against the nine-product kernel under the PC-100 limits, the seeded twin against the injected-noise
path, the alignment rule of the entry points, and the routing (agent -> 6, sampler_products = 9 -> the default sampler's bits, class
default nine)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import f64_reference as fr
from oracle import genpose_oracle as go

from test_gpu_bf16x9 import GATE_VS_F32, _inputs, _net
from test_gpu_f64_score import CHAIN_SHAPES, _cell, _first_pc
from test_gpu_fullsize import PC100_ROT_MAX, PC100_ROT_P999, PC100_TRANS_RTOL, _pose_errors
from test_gpu_x9_alignment import _off_by_one_float

X6, X9, F32 = "pc_step_chain_kernel<bf16x9,6>", "pc_step_chain_kernel<bf16x9>", "pc_step_chain_kernel<2>"


def _sampler(net, B, K, n, groups, arith, **kw):
    """arith: 6 | 9 (the split-bf16 trunk with that many products) | 'f32mfma'"""
    from genpose_amd.samplers import PCSampler
    if arith == "f32mfma":
        smp = PCSampler(net, B, K, n, "cuda", groups=groups, tile=128, trunk="f32mfma", **kw)
    else:
        smp = PCSampler(net, B, K, n, "cuda", groups=groups, tile=128, trunk="bf16x9", products=arith, **kw)
    assert smp.tile == 128 and smp.kernel_name == {6: X6, 9: X9, "f32mfma": F32}[arith]  # the test must not silently measure another kernel
    assert smp.products == (arith if arith != "f32mfma" else None)
    return smp


@pytest.mark.parametrize("which", fr.WEIGHTS)
def test_first_evaluation_under_the_float64_rule(which):
    """The float64 rule, unchanged (MARGIN = 3 x e_oracle_cell; no exception is granted), with the nine-product kernel printed beside;
    and on the same rows, per block over the same shape set, at most GATE_VS_F32 x the fp32 chain kernel's error."""
    first = lambda kernel, **kw: (lambda B, K, sc: _first_pc(which, "score", B, K, sc, kernel, tile=128, **kw))
    six, nine, f32 = first(X6, trunk="bf16x9", products=6), first(X9, trunk="bf16x9"), first(F32, trunk="f32mfma")
    bad = _cell("pc first evaluation", "128 bf16x9,6", which, "score", 1.0, CHAIN_SHAPES, six, nine)
    assert not bad, bad
    worst = {6: [0.0] * 3, 32: [0.0] * 3}
    for B, K in CHAIN_SHAPES:
        for sc in fr.POSE_SCALES:
            c = fr.case(which, "score", B, K, sc, 1.0)
            for key, fn in ((6, six), (32, f32)):
                worst[key] = [max(a, b) for a, b in zip(worst[key], fr.errors(fn(B, K, sc), c, "score")["score"])]
    for j in range(3):
        print(f"x6 vs fp32 chain | {which:7s} | head {j} | fp32 chain {worst[32][j]:.2e} | six {worst[6][j]:.2e} | ratio {worst[6][j] / worst[32][j]:.3f}")
    assert all(e6 <= GATE_VS_F32 * e32 for e6, e32 in zip(worst[6], worst[32])), worst


@pytest.mark.parametrize("B,K,groups", [(3, 43, 1), (45, 50, 1), (128, 50, 2)])
def test_ragged_and_grouped_against_fp32_chain(B, K, groups):
    """A ragged last workgroup (129 and 2 250 rows) and two batches per launch: 30 steps against the fp32 chain kernel - the tolerance the
    nine-product kernel is held to (tests/test_gpu_bf16x9.py); a captured chain and two replays give the launched bits; a batch computes
    alone what it computes inside a two-batch launch."""
    net = _net()
    n = 30
    feat, centre, x0, z1, z2 = (t.cuda() for t in _inputs(B, K, n, B + K))
    cvec = net.cloud_embed(feat)
    out = {}
    for arith in ("f32mfma", 6):
        smp = _sampler(net, B, K, n, groups, arith, record_traj=True, use_graph=False)
        xs, mx = smp.run(cvec, centre, x0, z1, z2)
        torch.cuda.synchronize()
        out[arith] = (xs.clone(), mx.clone())
    sc = float(out["f32mfma"][1].abs().max())
    np.testing.assert_allclose(out[6][1].cpu().numpy(), out["f32mfma"][1].cpu().numpy(), rtol=0, atol=2e-5 * sc)
    np.testing.assert_allclose(out[6][0].cpu().numpy(), out["f32mfma"][0].cpu().numpy(), rtol=0, atol=2e-5 * float(out["f32mfma"][0].abs().max()))
    assert not torch.equal(out[6][1], out["f32mfma"][1])
    # replays: the captured chain, then two replays of it
    g = _sampler(net, B, K, n, groups, 6, record_traj=True)
    for rep in range(3):
        xs, mx = g.run(cvec, centre, x0, z1, z2)
        torch.cuda.synchronize()
        assert g.graph is not None and g.captures == 1
        assert torch.equal(mx, out[6][1]) and torch.equal(xs, out[6][0]), rep
    if groups == 2:
        B1, R1 = B // 2, B // 2 * K
        for b in range(2):
            one = _sampler(net, B1, K, n, 1, 6, use_graph=False)
            _, m1 = one.run(cvec[b * B1:(b + 1) * B1], centre[b * B1:(b + 1) * B1], x0[b * R1:(b + 1) * R1], z1[:, b * R1:(b + 1) * R1].contiguous(),
                            z2[:, b * R1:(b + 1) * R1].contiguous())
            torch.cuda.synchronize()
            assert torch.equal(m1, out[6][1][b * R1:(b + 1) * R1]), b


def test_coupling_statistic_from_outside():
    """gn_ext (a sharded batch's per-step sums of |score| handed in from outside): the uncoupled result, and the fp32 chain kernel's within
    its tolerance - tests/test_gpu_bf16x9.py's check on the six-product kernel."""
    net = _net()
    B, K, n, groups = 128, 50, 12, 2
    feat, centre, x0, z1, z2 = (t.cuda() for t in _inputs(B, K, n, 77))
    cvec = net.cloud_embed(feat)
    res = {}
    for arith in ("f32mfma", 6):
        for coupled in (False, True):
            smp = _sampler(net, B, K, n, groups, arith, use_graph=False)
            smp.cvec.copy_(cvec), smp.centre.copy_(centre), smp.x.copy_(x0), smp.z1.copy_(z1), smp.z2.copy_(z2)
            if coupled:
                smp.gn_ext, smp.gn_rows = torch.zeros(n, groups, device="cuda"), B * K // groups
            for i in range(n + 1):
                smp.launch_step(i)
                if coupled and i < n:
                    torch.sum(smp.partials[i].view(groups, -1), dim=1, out=smp.gn_ext[i])
            torch.cuda.synchronize()
            res[arith, coupled] = smp.mean_x.cpu().clone()
    sc = float(res[6, False].abs().max())
    np.testing.assert_allclose(res[6, True].numpy(), res[6, False].numpy(), rtol=0, atol=1e-5 * sc)
    sc = float(res["f32mfma", True].abs().max())
    np.testing.assert_allclose(res[6, True].numpy(), res["f32mfma", True].numpy(), rtol=0, atol=2e-5 * sc)


def test_pc100_against_nine_products():
    """PC-100 on 3 x 50 rows, the same draws: six products against nine within the PC-100 limits of the fp32 tests."""
    net = _net()
    B, K, n = 3, 50, 100
    feat, centre, x0, z1, z2 = (t.cuda() for t in _inputs(B, K, n, 2025))
    x0 = x0 * (float(go.ve_sigma(1.0)) / 50.0)  # the prior's scale at t = 1
    cvec = net.cloud_embed(feat)
    out = {}
    for arith in (9, 6):
        out[arith] = _sampler(net, B, K, n, 1, arith).run(cvec, centre, x0, z1, z2)[1].cpu().numpy().copy()
    p999, mx, trans = _pose_errors(out[6], out[9])
    print(f"PC-100, 3 clouds x 50, six vs nine products: rotation p99.9 {p999:.2e} max {mx:.2e}, translation (rel) {trans:.2e} "
          f"(limits {PC100_ROT_P999:.0e} / {PC100_ROT_MAX:.0e} / {PC100_TRANS_RTOL:.0e})")
    assert np.isfinite(out[6]).all() and not np.array_equal(out[6], out[9])
    assert p999 < PC100_ROT_P999 and mx < PC100_ROT_MAX and trans < PC100_TRANS_RTOL


def test_routing():
    """A score-model PC agent at a chain-plan size runs six products; sampler_products = 9 gives the bits of a directly built default
    PCSampler; the class default is nine; anywhere but the bf16x9 trunk the argument is ignored."""
    from genpose_amd.config import get_config, sampler_products_of
    from genpose_amd.posenet_agent import PoseNet
    from genpose_amd.samplers import PCSampler
    B, K, n = 640, 50, 3
    feat, centre, x0, z1, z2 = (t.cuda() for t in _inputs(B, K, n, 31))
    got = {}
    for sp in ("auto", 9, 6):
        cfg = get_config(posenet_mode="score", sampler_mode=["pc"], sampling_steps=n, sampler_products=sp)
        agent = PoseNet(cfg)
        agent.load_state_dict(go.make_state_dict(0, "score"))
        net = agent.net
        _, res = net.sample({"pts_feat": feat, "pts_center": centre, "_repeat": K}, "pc", init_x=x0, noise=(z1, z2), return_process=False)
        torch.cuda.synchronize()
        smp = net.last_sampler
        want = 9 if sp == 9 else 6
        assert smp.tile == 128 and smp.products == want == sampler_products_of(cfg) and smp.kernel_name == (X6 if want == 6 else X9), (sp, smp.kernel_name)
        got[sp] = res.clone()
    snet = net.pose_score_net
    direct = PCSampler(snet, B, K, n, "cuda", record_traj=False)  # the class default
    assert direct.products == 9 and direct.kernel_name == X9 and direct.tile == 128
    _, ref = direct.run(snet.cloud_embed(feat), centre, x0, z1, z2)
    torch.cuda.synchronize()
    assert torch.equal(got[9], ref) and torch.equal(got["auto"], got[6]) and not torch.equal(got[6], got[9])
    # ignored where the bf16x9 trunk does not apply
    assert PCSampler(snet, 64, 50, n, "cuda", products=6).products is None
    assert PCSampler(snet, B, K, n, "cuda", trunk="f32mfma", products=6).kernel_name == F32
    assert sampler_products_of(get_config(posenet_mode="energy", sampler_mode=["pc"], sampling_steps=n)) == 9
    assert sampler_products_of(get_config(posenet_mode="score", sampler_mode=["ode"])) == 9
    with pytest.raises(ValueError):
        PCSampler(snet, B, K, n, "cuda", products=8)
    with pytest.raises(ValueError):
        sampler_products_of(get_config(sampler_products=8))


@pytest.mark.parametrize("G,B1,K", [(2, 64, 50), (1, 3, 43)])
def test_seeded_kernel_equals_the_injected_noise_path(G, B1, K):
    """pc_step_chain_seeded_kernel_bf16x6 against the unseeded six-product kernel on gp_pc_noise_fill's buffers for the same seed state:
    poses, trajectory and partial sums bit for bit (tests/test_gpu_seeded_noise.py's identity)."""
    from genpose_amd.samplers import pc_noise_fill
    net = _net()
    n, seed = 6, 0x5EED
    feat, centre, x0, _, _ = (t.cuda() for t in _inputs(G * B1, K, 1, 17 * G + B1))
    cvec = net.cloud_embed(feat)
    seeded = _sampler(net, G * B1, K, n, G, 6, record_traj=True, seed=seed)
    plain = _sampler(net, G * B1, K, n, G, 6, record_traj=True)
    assert seeded.z1 is None
    xs, m = seeded.run(cvec, centre, x0, run_index=5)
    z1, z2 = pc_noise_fill(seed, 5, n, G * B1 * K, "cuda")
    xs_p, m_p = plain.run(cvec, centre, x0, z1, z2)
    torch.cuda.synchronize()
    assert torch.isfinite(m).all() and torch.equal(m, m_p) and torch.equal(xs, xs_p) and torch.equal(seeded.partials, plain.partials)


@pytest.mark.parametrize("which", ["cvec", "tvec_all"])
@pytest.mark.parametrize("seeded", [False, True])
def test_misaligned_staged_operand_is_refused(seeded, which):
    """gp_pc_step_bf16x6 and gp_pc_step_bf16x6_seeded refuse a misaligned cvec / tvec_all with GP_EINVAL before anything is launched."""
    from genpose_amd._lib import GenposeHipError
    smp = _sampler(_net(), 3, 43, 2, 1, 6, use_graph=False, **({"seed": 1} if seeded else {}))
    if seeded:
        smp._write_seed_state(0, None)
    else:
        smp.z1.zero_(), smp.z2.zero_()
    smp.cvec.zero_(), smp.centre.zero_(), smp.x.zero_()
    smp.launch_step(0)  # aligned: accepted
    torch.cuda.synchronize()
    setattr(smp, which, _off_by_one_float(getattr(smp, which)))
    with pytest.raises(GenposeHipError, match="GP_EINVAL"):
        smp.launch_step(0)
    torch.cuda.synchronize()
