"""GPU: the opt-in seeded noise of the PC sampler (csrc/philox.h, csrc/noise.hip, PCSampler(seed=)).  The device generator equals the
numpy restatement (tests/philox_reference.py) bit for bit in its raw words and to the transcendental functions' round-off in its normals;
a seeded sampler equals the EXISTING injected-noise path fed with gp_pc_noise_fill's buffers bit for bit under every served plan - so
the oracle parity of the seeded path is the injected-noise tests' (test_gpu_sampler / _chain / _bf16x9 / _headsplit / _tile32); a row's
draws do not depend on the launch's layout; the seed state is read at run time, not frozen into the captured graph."""
import os
import socket

import numpy as np
import pytest
import torch

import philox_reference as pr

pytestmark = pytest.mark.gpu

HS = 0x100  # GP_PLAN_HEADSPLIT
SEED = 0xC0FFEE1234567890  # (bit 63 set: the whole 64 bits travel)

# Largest |device - numpy| over the 4.7e6 normals of test_normals_against_the_restatement (logf / sincosf of the device library against
# numpy's float32 log / sin / cos; the uniforms and sqrt are exact on both sides).  Measured on an MI355X on 2026-10-17: 4.768e-07
# (one ulp at |z| in [4, 8), two at [2, 4)).
NORMALS_MAX_ABS_DIFF_MEASURED = 4.768e-07


@pytest.fixture(scope="module")
def net():
    from genpose_amd.scorenet import ScoreNetHIP
    from genpose_amd.weights_synth import make_state_dict
    return ScoreNetHIP(make_state_dict(0, "score"), "cuda")


def _dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def test_raw_words_equal_the_published_generator():
    """10^5 counters through gp_philox_raw: the layout's counters for random field tuples - rows above 2^32, the last step of a 500-step
    schedule, both streams, all blocks - and raw random counters; every word equals the numpy restatement."""
    from genpose_amd.samplers import philox_raw
    rng = np.random.default_rng(3)
    n = 50_000
    rows = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    rows[:1000] += np.uint64(1 << 32)
    rows[1000:1010] = np.uint64((1 << 64) - 1)
    steps = rng.integers(0, 500, n, dtype=np.uint64)
    steps[:2000] = 499
    ctr, key = pr.pack(rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1), rng.integers(0, 1 << 32, n, dtype=np.uint64), steps,
                       rng.integers(0, 2, n, dtype=np.uint64), rng.integers(0, 3, n, dtype=np.uint64), rows)
    ctr = np.concatenate([ctr, rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64).astype(np.uint32)])
    key = np.concatenate([key, rng.integers(0, 1 << 32, (n, 2), dtype=np.uint64).astype(np.uint32)])
    ctr[-1], key[-1] = 0xFFFFFFFF, 0xFFFFFFFF
    ctr[-2], key[-2] = 0, 0
    assert (ctr[:n, 1] > 0).sum() >= 1000 and len(ctr) == 100_000
    got = philox_raw(_dev_u32(ctr), _dev_u32(key)).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, pr.philox4x32_10(ctr, key))
    assert [hex(int(v)) for v in got[-2]] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]


def test_normals_against_the_restatement():
    """gp_pc_noise_fill against the restatement's float32 normals (bound: 4 x the difference measured once, see the constant), the CPU
    test's statistics with the CPU test's bounds on the device output, and a row base above 2^32."""
    from genpose_amd.samplers import pc_noise_fill
    from test_philox_cpu import STAT_ROWS, STAT_RUN, STAT_SEED, STAT_STEPS
    z1, z2 = (t.cpu().numpy() for t in pc_noise_fill(STAT_SEED, STAT_RUN, STAT_STEPS, STAT_ROWS, "cuda"))
    r1, r2 = pr.noise(STAT_SEED, STAT_RUN, STAT_STEPS, STAT_ROWS)
    diff = max(np.abs(z1 - r1).max(), np.abs(z2 - r2).max())
    print(f"normals: max |device - numpy| = {diff:.3e} over {z1.size + z2.size} values; max |z| = {max(np.abs(z1).max(), np.abs(z2).max()):.4f}")
    z1n = pc_noise_fill(STAT_SEED + 1, STAT_RUN, STAT_STEPS, STAT_ROWS, "cuda")[0].cpu().numpy()
    res = pr.statistics(z1, z2, z1n)
    for name, val, bound in res:
        print(f"{name}: {val:.3e} (bound {bound:.3e})")
    assert diff <= 4 * NORMALS_MAX_ABS_DIFF_MEASURED
    assert np.isfinite(z1).all() and max(np.abs(z1).max(), np.abs(z2).max()) <= pr.Z_MAX * (1 + 1e-6)
    assert not [(n, v, b) for n, v, b in res if not v < b]
    base = (1 << 40) + 12345
    h1, h2 = (t.cpu().numpy() for t in pc_noise_fill(SEED, 7, 2, 4096, "cuda", row_base=base, step0=498))
    q1, q2 = pr.noise(SEED, 7, 2, 4096, row_base=base, step0=498)
    assert max(np.abs(h1 - q1).max(), np.abs(h2 - q2).max()) <= 4 * NORMALS_MAX_ABS_DIFF_MEASURED


def _inputs(G, B1, K, seed):
    gen = torch.Generator().manual_seed(seed)
    feat = torch.randn(G * B1, 1024, generator=gen).abs()
    centre = torch.randn(G * B1, 3, generator=gen) * 0.3
    x0 = torch.randn(G * B1 * K, 9, generator=gen) * 50.0
    if G > 1:
        x0[B1 * K:] *= 0.2  # the batches see very different gradient norms
    return feat.cuda(), centre.cuda(), x0.cuda()


# (name, batches, clouds per batch, candidates, steps, plan, trunk): the shapes at which tests/test_gpu_chain.py, test_gpu_bf16x9.py,
# test_gpu_headsplit.py and test_gpu_tile32.py run these plans
PLANS = [
    ("16-row tiles", 1, 45, 50, 8, 16, None, "pc_step_kernel<16>"),
    ("32-row tiles", 2, 64, 50, 6, 32, None, "pc_step_kernel<32>"),
    ("64-row tiles", 2, 64, 50, 6, 64, None, "pc_step_kernel<64>"),
    ("head-split", 1, 6, 50, 25, 16 | HS, None, "pc_step_kernel<16,0,split>"),
    ("fp32 chain", 1, 45, 50, 8, 128, "f32mfma", "pc_step_chain_kernel<2>"),
    ("bf16x9 chain", 2, 64, 50, 6, 128, None, "pc_step_chain_kernel<bf16x9>"),
    ("bf16x9 chain, ragged", 1, 3, 43, 6, 128, "bf16x9", "pc_step_chain_kernel<bf16x9>"),
]


@pytest.mark.parametrize("name,G,B1,K,n,plan,trunk,kernel", PLANS, ids=[p[0] for p in PLANS])
def test_seeded_sampler_equals_the_injected_noise_path(net, name, G, B1, K, n, plan, trunk, kernel):
    """The identity that carries parity: a seeded sampler (noise drawn in the step kernels, whole schedule, captured graph) against
    the unseeded sampler of the same plan run on gp_pc_noise_fill's buffers for the same seed state: final poses, trajectory and
    per-step partial sums are bit-identical."""
    from genpose_amd.samplers import PCSampler, pc_noise_fill
    feat, centre, x0 = _inputs(G, B1, K, 17 * G + B1)
    cvec = net.cloud_embed(feat)
    R = G * B1 * K
    seeded = PCSampler(net, G * B1, K, n, "cuda", record_traj=True, groups=G, tile=plan, trunk=trunk, seed=SEED)
    plain = PCSampler(net, G * B1, K, n, "cuda", record_traj=True, groups=G, tile=plan, trunk=trunk)
    assert seeded.kernel_name == plain.kernel_name == kernel and seeded.z1 is None and seeded.z2 is None
    xs, m = seeded.run(cvec, centre, x0, run_index=5)
    z1, z2 = pc_noise_fill(SEED, 5, n, R, "cuda")
    xs_p, m_p = plain.run(cvec, centre, x0, z1, z2)
    torch.cuda.synchronize()
    assert seeded.graph is not None and torch.isfinite(m).all()
    assert torch.equal(m, m_p), f"{name}: mean_x differs by {float((m - m_p).abs().max()):.3e}"
    assert torch.equal(xs, xs_p), f"{name}: trajectory differs by {float((xs - xs_p).abs().max()):.3e}"
    assert torch.equal(seeded.partials, plain.partials), name
    # and the draws moved the chain: another run index is another sample
    _, m_other = seeded.run(cvec, centre, x0, run_index=6)
    assert not torch.equal(m_other, m_p)


def test_fill_window_equals_the_larger_fill():
    from genpose_amd.samplers import pc_noise_fill
    a1, a2 = pc_noise_fill(SEED, 2, 5, 1000, "cuda", row_base=77)
    b1, b2 = pc_noise_fill(SEED, 2, 2, 130, "cuda", row_base=77, step0=3, row0=400)
    c1, c2 = pc_noise_fill(SEED, 2, 2, 130, "cuda", row_base=477, step0=3)
    assert torch.equal(a1[3:, 400:530], b1) and torch.equal(a2[3:, 400:530], b2) and torch.equal(b1, c1) and torch.equal(b2, c2)
    assert not torch.equal(a1, a2)


def test_batches_of_a_launch_draw_what_they_draw_alone(net):
    """Request batching: batch g of a G-batch launch equals a stand-alone seeded sampler on that batch with row_base = g x rows per
    batch, bit for bit (the same plan on both sides: the per-batch norm is reduced from the same partial sums in the same order)."""
    from genpose_amd.samplers import PCSampler
    G, B1, K, n = 3, 16, 10, 6
    R1 = B1 * K
    feat, centre, x0 = _inputs(G, B1, K, 5)
    cvec = net.cloud_embed(feat)
    _, m = PCSampler(net, G * B1, K, n, "cuda", groups=G, tile=32, seed=SEED).run(cvec, centre, x0, run_index=1)
    m = m.clone()
    for g in range(G):
        cl, rows = slice(g * B1, (g + 1) * B1), slice(g * R1, (g + 1) * R1)
        alone = PCSampler(net, B1, K, n, "cuda", tile=32, seed=SEED, row_base=g * R1)
        _, ma = alone.run(cvec[cl].contiguous(), centre[cl].contiguous(), x0[rows].contiguous(), run_index=1)
        assert torch.equal(ma, m[rows]), f"batch {g}"
        if g:  # and the base matters: without it batch g draws batch 0's values
            _, mb = alone.run(cvec[cl].contiguous(), centre[cl].contiguous(), x0[rows].contiguous(), run_index=1, row_base=0)
            assert not torch.equal(mb, m[rows])


def test_run_index_and_reseeding_follow_through_the_captured_graph(net):
    """Consecutive runs differ; a pinned run index reproduces a run; a new seed written to the seed state is followed by the SAME
    captured graph (nothing was frozen at capture)."""
    from genpose_amd.samplers import PCSampler
    B, K, n = 8, 10, 12
    feat, centre, x0 = _inputs(1, B, K, 9)
    cvec = net.cloud_embed(feat)
    smp = PCSampler(net, B, K, n, "cuda", seed=11)
    first = smp.run(cvec, centre, x0)[1].clone()
    assert smp.last_run_index == 0
    graph = smp.graph
    second = smp.run(cvec, centre, x0)[1].clone()
    assert smp.last_run_index == 1 and not torch.equal(first, second)
    assert torch.equal(smp.run(cvec, centre, x0, run_index=0)[1], first)
    assert torch.equal(smp.run(cvec, centre, x0, run_index=1)[1], second)
    smp.reseed(12)
    other = smp.run(cvec, centre, x0)[1].clone()
    assert graph is not None and smp.graph is graph and not torch.equal(other, first)
    fresh = PCSampler(net, B, K, n, "cuda", seed=12, use_graph=False)
    assert torch.equal(fresh.run(cvec, centre, x0)[1], other)


def test_seeded_sampler_holds_no_noise_buffers(net):
    """12 800 rows x 100 steps: the unseeded sampler's two [100, 12800, 9] fp32 buffers (92 MB) are not there."""
    from genpose_amd.samplers import PCSampler
    B, K, n = 256, 50, 100

    def footprint(**kw):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        smp = PCSampler(net, B, K, n, "cuda", tile=32, **kw)
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated() - before, smp

    footprint()  # (whatever the first construction caches on the network is allocated now)
    plain, smp_p = footprint()
    seeded, smp_s = footprint(seed=1)
    two_buffers = 2 * n * B * K * 9 * 4
    assert smp_s.z1 is None and smp_s.z2 is None and smp_p.z1.numel() * 4 * 2 == two_buffers
    print(f"sampler footprint: unseeded {plain / 2**20:.1f} MiB, seeded {seeded / 2**20:.1f} MiB")
    assert seeded <= plain - two_buffers + (2 << 20)  # one allocator block (2 MiB) of slack


def test_refusals(net):
    from genpose_amd.samplers import PCSampler
    feat, centre, x0 = _inputs(1, 8, 10, 1)
    cvec = net.cloud_embed(feat)
    smp = PCSampler(net, 8, 10, 4, "cuda", seed=3)
    z = torch.zeros(4, 80, 9, device="cuda")
    with pytest.raises(ValueError, match="seeded sampler"):
        smp.run(cvec, centre, x0, z_langevin=z, z_predictor=z)
    with pytest.raises(ValueError, match="seed="):
        PCSampler(net, 8, 10, 4, "cuda").run(cvec, centre, x0, run_index=0)
    with pytest.raises(NotImplementedError, match="bf16x3"):
        PCSampler(net, 128, 50, 4, "cuda", precision="bf16x3", seed=3)
    with pytest.raises(NotImplementedError, match="energy"):
        PCSampler(net, 8, 10, 4, "cuda", model="energy", seed=3)
    with pytest.raises(ValueError):
        smp.run(cvec, centre, x0, run_index=1 << 32)


def test_config_flag_reaches_the_sampler():
    """get_config(sampler_seed=): GFObjectPose.sample builds a seeded sampler (part of its cache key); equal seeds give equal poses,
    explicit noise is refused."""
    from genpose_amd import synth
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    from genpose_amd.weights_synth import make_state_dict
    assert get_config().sampler_seed is None
    B, K, n = 3, 6, 8
    pts = torch.from_numpy(synth.make_batch(B, start=500)).cuda()
    prior = torch.randn(B * K, 9, generator=torch.Generator().manual_seed(1))

    def pred(seed, **kw):
        a = PoseNet(get_config(posenet_mode="score", sampler_mode=["pc"], sampling_steps=n, sampler_seed=seed))
        a.load_state_dict(make_state_dict(0, "score"))
        a.net.prior_fn = lambda shape, T=1.0: prior * (0.01 * 5000.0 ** T)
        out = a.pred_func({"pts": pts, "pts_center": pts.mean(dim=1)}, K, save_path=None, **kw)
        return out.clone(), a.net.last_sampler

    p1, s1 = pred(21)
    p2, _ = pred(21)
    p3, _ = pred(22)
    assert s1.seed == 21 and s1.z1 is None and torch.isfinite(p1).all()
    assert torch.equal(p1, p2) and not torch.equal(p1, p3)
    with pytest.raises(ValueError):
        pred(21, noise=(torch.zeros(n, B * K, 9, device="cuda"),) * 2)


SB, SK, SN = 8, 10, 12


def _shard_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        from genpose_amd.samplers import PCSampler
        from genpose_amd.scorenet import ScoreNetHIP
        from genpose_amd.weights_synth import make_state_dict
        net = ScoreNetHIP(make_state_dict(0, "score"), "cuda")
        feat, centre, x0 = _inputs(2, SB // 2, SK, 31)
        cvec = net.cloud_embed(feat)
        bs = SB // world
        cl, rows = slice(rank * bs, (rank + 1) * bs), slice(rank * bs * SK, (rank + 1) * bs * SK)
        smp = PCSampler(net, bs, SK, SN, "cuda", coupling_group=dist.group.WORLD, seed=SEED)
        assert smp.row_base == rank * bs * SK
        _, m = smp.run(cvec[cl].contiguous(), centre[cl].contiguous(), x0[rows].contiguous(), run_index=4)
        torch.cuda.synchronize()
        np.save(os.path.join(out_dir, f"seeded_{rank}.npy"), m.cpu().numpy())
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_shards_draw_the_unsharded_batch(net, tmp_path):
    """Two processes on the one device (gloo), each holding half of a batch with cross-rank coupling and the default row base
    rank x rows per shard: together they reproduce the unsharded seeded batch - to the tolerance tests/test_gpu_coupled.py holds the
    injected-noise path to (1e-4 of the scale: the all-reduced norm sum is formed in another order); with shard-local draws (both
    shards at row base 0) the second shard would be another sample.  coupling_group with groups > 1 is refused."""
    import torch.multiprocessing as mp
    from genpose_amd.samplers import PCSampler
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_shard_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    feat, centre, x0 = _inputs(2, SB // 2, SK, 31)
    cvec = net.cloud_embed(feat)
    full = PCSampler(net, SB, SK, SN, "cuda", seed=SEED).run(cvec, centre, x0, run_index=4)[1].cpu().numpy()
    shards = np.concatenate([np.load(tmp_path / f"seeded_{r}.npy") for r in range(2)])
    scale = np.abs(full).max()
    print(f"sharded vs unsharded seeded batch: max diff {np.abs(shards - full).max():.3e} (scale {scale:.3e})")
    np.testing.assert_allclose(shards, full, rtol=0, atol=1e-4 * scale)
    with pytest.raises(NotImplementedError, match="groups > 1"):
        PCSampler(net, SB, SK, SN, "cuda", groups=2, coupling_group=object(), seed=SEED)
