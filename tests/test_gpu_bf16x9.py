"""GPU: the exact-product split-bf16 chain plan of the score model's PC step (csrc/trunk_bf16x9.hip, the default for 128-row workgroups)
against the fp32-MFMA chain kernel it replaces (PCSampler(trunk='f32mfma')) and against fp64.

Accuracy gate: the first score evaluation's max error over the score's scale against an fp64 evaluation of the network is at most 1.5x
the fp32 chain kernel's on the same rows; PC-100 over the benched 640 clouds (same draws) within the PC-100 tolerance of the fp32 tests.
Also: cross-rank coupling (gn_ext), a ragged last workgroup, several batches per launch, replays to the same bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import genpose_oracle as go

from test_gpu_fullsize import PC100_ROT_MAX, PC100_ROT_P999, PC100_TRANS_RTOL, _pose_errors

GATE_VS_F32 = 1.5


def _net():
    from genpose_amd.scorenet import ScoreNetHIP
    return ScoreNetHIP(go.make_state_dict(0, "score"), "cuda")


def _inputs(B, K, n, seed):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(B, 1024, generator=g).abs()
    centre = torch.randn(B, 3, generator=g) * 0.3
    x0 = torch.randn(B * K, 9, generator=g) * 50.0
    z1, z2 = torch.randn(n, B * K, 9, generator=g), torch.randn(n, B * K, 9, generator=g)
    return feat, centre, x0, z1, z2


def _sampler(net, B, K, n, groups, trunk, **kw):
    from genpose_amd.samplers import PCSampler
    smp = PCSampler(net, B, K, n, "cuda", groups=groups, tile=128, trunk=trunk, **kw)
    assert smp.tile == 128 and smp.kernel_name.startswith("pc_step_chain_kernel")
    assert smp.kernel_name == ("pc_step_chain_kernel<bf16x9>" if trunk == "bf16x9" else "pc_step_chain_kernel<2>")
    return smp


def test_default_chain_plan_is_bf16x9():
    from genpose_amd.samplers import PCSampler
    net = _net()
    assert PCSampler(net, 640, 50, 4, "cuda", groups=10).kernel_name == "pc_step_chain_kernel<bf16x9>"
    assert PCSampler(net, 64, 50, 4, "cuda").kernel_name == "pc_step_kernel<16>"  # tile plans keep their kernels
    assert PCSampler(net, 640, 50, 4, "cuda", groups=10, model="energy", tile=128).kernel_name == "pc_step_chain_kernel<2,energy>"
    with pytest.raises(ValueError):
        PCSampler(net, 640, 50, 4, "cuda", groups=10, trunk="f16")


def test_first_evaluation_against_fp64():
    """The gate: max |score - fp64| / max |fp64| of the first evaluation, 6 400 rows in two batches of 128-row workgroups."""
    net = _net()
    B, K, n, groups = 128, 50, 2, 2
    feat, centre, x0, z1, z2 = _inputs(B, K, n, 5)
    cvec = net.cloud_embed(feat.cuda())
    first = {}
    for trunk in ("f32mfma", "bf16x9"):
        smp = _sampler(net, B, K, n, groups, trunk)
        smp.cvec.copy_(cvec), smp.centre.copy_(centre.cuda()), smp.x.copy_(x0.cuda()), smp.z1.copy_(z1.cuda()), smp.z2.copy_(z2.cuda())
        smp.launch_step(0)
        torch.cuda.synchronize()
        first[trunk] = smp.score.double().cpu()
    sd64 = {k: v.double() for k, v in go.make_state_dict(0, "score").items()}
    ref = go.score_forward(sd64, feat.repeat_interleave(K, 0).double(), x0.double(), torch.ones(B * K, 1, dtype=torch.float64))
    scale = float(ref.abs().max())
    e32 = float((first["f32mfma"] - ref).abs().max()) / scale
    e9 = float((first["bf16x9"] - ref).abs().max()) / scale
    print(f"first evaluation vs fp64, max error / score scale: fp32 chain {e32:.2e}, bf16x9 {e9:.2e} (ratio {e9 / e32:.2f})")
    assert e32 < 5e-6 and e9 <= GATE_VS_F32 * e32, (e32, e9)
    assert not torch.equal(first["f32mfma"], first["bf16x9"])  # (it IS a different arithmetic)


def test_pc100_benched_clouds_against_fp32_chain():
    """PC-100 over the 640 clouds bench.py times (ten 64-cloud batches per launch, the same draws): new kernel against the fp32 chain
    kernel, the PC-100 tolerance of the fp32 tests; graph replays give the same bits."""
    from genpose_amd import synth
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    agent = PoseNet(get_config(posenet_mode="score", sampler_mode=["pc"], sampling_steps=100))
    agent.load_state_dict(go.make_state_dict(0, "score"))
    agent.net._need_weights()
    G, B1, K, n = 10, 64, 50, 100
    pts = torch.cat([torch.from_numpy(synth.make_batch(B1, start=B1 * i)) for i in range(G)], dim=0).cuda()
    feat = agent.net.pts_encoder.forward(pts)
    snet = agent.net.pose_score_net
    cvec, centre = snet.cloud_embed(feat), pts.mean(dim=1)
    gen = torch.Generator().manual_seed(2024)
    x0 = (torch.randn(G * B1 * K, 9, generator=gen) * float(go.ve_sigma(1.0))).cuda()
    z1, z2 = torch.randn(n, G * B1 * K, 9, generator=gen).cuda(), torch.randn(n, G * B1 * K, 9, generator=gen).cuda()
    out = {}
    for trunk in ("f32mfma", "bf16x9"):
        smp = _sampler(snet, G * B1, K, n, G, trunk)
        a = smp.run(cvec, centre, x0, z1, z2)[1].clone()
        b = smp.run(cvec, centre, x0, z1, z2)[1]
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        out[trunk] = a.cpu().numpy()
    p999, mx, trans = _pose_errors(out["bf16x9"], out["f32mfma"])
    print(f"PC-100, 640 clouds x 50, bf16x9 vs fp32 chain: rotation p99.9 {p999:.2e} max {mx:.2e}, translation (rel) {trans:.2e} "
          f"(tolerance {PC100_ROT_P999:.0e} / {PC100_ROT_MAX:.0e} / {PC100_TRANS_RTOL:.0e})")
    assert p999 < PC100_ROT_P999 and mx < PC100_ROT_MAX and trans < PC100_TRANS_RTOL


@pytest.mark.parametrize("B,K,groups", [(3, 43, 1), (45, 50, 1), (128, 50, 2)])
def test_ragged_and_grouped_against_fp32_chain(B, K, groups):
    """A ragged last workgroup (129 and 2 250 rows) and two batches per launch: 30 steps against the fp32 chain kernel and the oracle."""
    net = _net()
    n = 30
    feat, centre, x0, z1, z2 = _inputs(B, K, n, B + K)
    cvec = net.cloud_embed(feat.cuda())
    out = {}
    for trunk in ("f32mfma", "bf16x9"):
        smp = _sampler(net, B, K, n, groups, trunk, record_traj=True)
        xs, mx = smp.run(cvec, centre.cuda(), x0.cuda(), z1.cuda(), z2.cuda())
        torch.cuda.synchronize()
        out[trunk] = (xs.cpu().clone(), mx.cpu().clone())
    sc = float(out["f32mfma"][1].abs().max())
    np.testing.assert_allclose(out["bf16x9"][1].numpy(), out["f32mfma"][1].numpy(), rtol=0, atol=2e-5 * sc)
    np.testing.assert_allclose(out["bf16x9"][0].numpy(), out["f32mfma"][0].numpy(), rtol=0, atol=2e-5 * float(out["f32mfma"][0].abs().max()))
    if groups == 1:
        _, oref = go.pc_sampler(lambda x, t: go.score_forward(go.make_state_dict(0, "score"), feat.repeat_interleave(K, 0), x, t), x0,
                                centre.repeat_interleave(K, 0), n, z1, z2)
        np.testing.assert_allclose(out["bf16x9"][1].numpy(), oref.numpy(), rtol=1e-3, atol=1e-3 * float(oref.abs().max()))


def test_coupling_statistic_from_outside():
    """The gn_ext path of a sharded batch (coupling_group): the per-step sums of |score| handed in from outside, as the all-reduce would,
    give the uncoupled result (one shard = the whole batch), on both trunks alike."""
    net = _net()
    B, K, n, groups = 128, 50, 12, 2
    feat, centre, x0, z1, z2 = _inputs(B, K, n, 77)
    cvec = net.cloud_embed(feat.cuda())
    res = {}
    for trunk in ("f32mfma", "bf16x9"):
        for coupled in (False, True):
            smp = _sampler(net, B, K, n, groups, trunk, use_graph=False)
            smp.cvec.copy_(cvec), smp.centre.copy_(centre.cuda()), smp.x.copy_(x0.cuda()), smp.z1.copy_(z1.cuda()), smp.z2.copy_(z2.cuda())
            if coupled:
                smp.gn_ext, smp.gn_rows = torch.zeros(n, groups, device="cuda"), B * K // groups
            for i in range(n + 1):
                smp.launch_step(i)
                if coupled and i < n:
                    torch.sum(smp.partials[i].view(groups, -1), dim=1, out=smp.gn_ext[i])
            torch.cuda.synchronize()
            res[trunk, coupled] = smp.mean_x.cpu().clone()
    for trunk in ("f32mfma", "bf16x9"):
        sc = float(res[trunk, False].abs().max())
        np.testing.assert_allclose(res[trunk, True].numpy(), res[trunk, False].numpy(), rtol=0, atol=1e-5 * sc)
    sc = float(res["f32mfma", True].abs().max())
    np.testing.assert_allclose(res["bf16x9", True].numpy(), res["f32mfma", True].numpy(), rtol=0, atol=2e-5 * sc)
