"""GPU: the whole fixed-step Heun solve in one launch (heun_solve_kernel<16|32|64>, gp_heun_solve_tile; HeunSampler(launches='single')).
The oracle is the per-launch chain on the same plan: the one-launch kernel runs the chain's arithmetic per row in the chain's order, so
the pose, the state and every trajectory state are equal BIT FOR BIT (torch.equal).  On top of that, one shape per tile against the float64
restatement (tests/heun_reference.py) at the tolerance tests/test_gpu_heun.py holds the chain to, and the refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import genpose_oracle as go

import heun_reference as hr

T0 = 0.55
# name -> (groups, clouds, K, tiles): 15 rows = less than one tile; 50 rows = a ragged last tile under every tile size (K = 10: a 32- or
# 64-row tile spans more clouds than the trunk stages, the epilogue's global-memory path); 2 groups x 32 rows = workgroups that end on a
# group's border
SHAPES = {
    "3x5": (1, 3, 5, (16,)),
    "5x10": (1, 5, 10, (16, 32, 64)),
    "2gx4x8": (2, 8, 8, (16, 32)),
}
CASES = [(name, tile) for name, s in SHAPES.items() for tile in s[3]]


@functools.lru_cache(maxsize=None)
def _net():
    from genpose_amd.scorenet import ScoreNetHIP
    return ScoreNetHIP(go.make_state_dict(0, "score"), "cuda")


@functools.lru_cache(maxsize=None)
def _inputs(B, K, T, seed=11):
    g = torch.Generator().manual_seed(seed + 1000 * B + K)
    feat = torch.randn(B, 1024, generator=g).abs()
    centre = torch.randn(B, 3, generator=g) * 0.3
    x0 = torch.randn(B * K, 9, generator=g) * float(hr.sigma(T))
    return _net().cloud_embed(feat.cuda()), centre.cuda(), x0.cuda()


def _pair(name, tile, n, **kw):
    from genpose_amd.samplers import HeunSampler
    groups, B, K, tiles = SHAPES[name]
    t = ctypes.c_int(0)
    from genpose_amd import _lib
    assert _lib.lib().gp_heun_layout(tile, groups, B // groups, K, ctypes.byref(t)) == 0 and t.value == tile
    chain = HeunSampler(_net(), B, K, n, "cuda", groups=groups, tile=tile, **kw)
    single = HeunSampler(_net(), B, K, n, "cuda", groups=groups, tile=tile, launches="single", **kw)
    assert chain.kernel_name == f"heun_step_kernel<{tile}>" and single.kernel_name == f"heun_solve_kernel<{tile}>"
    assert chain.launches == "chain" and single.launches == "single" and single.tile == chain.tile == tile
    return chain, single


def _run(smp, cvec, centre, x0, **kw):
    xs, pose = smp.run(cvec, centre, x0, **kw)
    torch.cuda.synchronize()
    return (None if xs is None else xs.clone()), pose.clone(), smp.x.clone()


def _assert_same(a, b, what):
    for u, v, part in zip(a, b, ("trajectory", "pose", "x")):
        assert (u is None) == (v is None), (what, part)
        if u is not None:
            assert torch.isfinite(u).all(), (what, part)
            assert torch.equal(u, v), f"{what} {part}: {int((u != v).sum())} of {u.numel()} words differ, max |diff| {float((u - v).abs().max()):.3e}"


@pytest.mark.parametrize("record_traj", [True, False])
@pytest.mark.parametrize("grid", ["geometric", "edm"])
@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("n", [1, 6])
@pytest.mark.parametrize("name,tile", CASES)
def test_one_launch_equals_the_chain_bit_for_bit(name, tile, n, denoise, grid, record_traj):
    groups, B, K, _ = SHAPES[name]
    chain, single = _pair(name, tile, n, denoise=denoise, grid=grid, record_traj=record_traj)
    inp = _inputs(B, K, T0)
    ref, got = _run(chain, *inp, T0=T0), _run(single, *inp, T0=T0)
    _assert_same(got, ref, f"{name} tile {tile} N={n} denoise={denoise} {grid}")
    assert (got[0] is not None) == record_traj
    assert not torch.equal(got[1], inp[2])  # (the solve did move the rows)
    st = single.last_stats
    assert st["device_launches"] == 1 and st["kernel"] == f"heun_solve_kernel<{tile}>"
    assert st["launches"] == chain.last_stats["launches"] == single.nlaunch == 2 * n + 1 + int(denoise) and st["nfev"] == chain.last_stats["nfev"]
    assert "device_launches" not in chain.last_stats and single.captures == 1


@pytest.mark.parametrize("name,tile", [("5x10", 32), ("2gx4x8", 16)])
def test_a_second_replay_follows_run_time_T0(name, tile):
    """The same captured graph at another T0 (the schedule and the time table are device buffers): the chain's bits again, one capture."""
    groups, B, K, _ = SHAPES[name]
    chain, single = _pair(name, tile, 6, record_traj=True)
    a = _inputs(B, K, T0)
    _assert_same(_run(single, *a, T0=T0), _run(chain, *a, T0=T0), f"{name} first run")
    b = _inputs(B, K, 0.15, seed=12)
    got, ref = _run(single, *b, T0=0.15), _run(chain, *b, T0=0.15)
    _assert_same(got, ref, f"{name} replay at T0 = 0.15")
    assert single.captures == 1 and chain.captures == 1
    assert not torch.equal(got[1], _run(single, *b, T0=0.2)[1]) and single.captures == 1  # (T0 does reach the kernel)


@pytest.mark.parametrize("plan", ["tile16", "tile32", "tile64"])
def test_against_the_float64_restatement(plan):
    """tests/test_gpu_heun.py's reference (heun_reference.py driving the oracle's score network in float64), shapes and tolerance
    (rtol = atol = 1e-3), N = 6, T0 = 0.55."""
    import test_gpu_heun as th
    from genpose_amd.samplers import HeunSampler
    B, K, tile, _ = th.PLANS[plan]
    assert th.N_STEPS == 6 and th.RTOL == th.ATOL == 1e-3
    traj_ref, _, den_ref = th._reference(B, K, T0, "geometric")
    feat, centre, x0 = th._inputs(B, K, T0)
    smp = HeunSampler(_net(), B, K, th.N_STEPS, "cuda", tile=tile, record_traj=True, launches="single")
    assert smp.kernel_name == f"heun_solve_kernel<{tile}>"
    xs, pose = smp.run(_net().cloud_embed(feat.cuda()), centre.cuda(), x0.cuda(), T0=T0)
    th._assert_close(xs.permute(1, 0, 2).cpu().numpy(), traj_ref, f"one launch {plan} trajectory")
    th._assert_close(pose.cpu().numpy(), den_ref, f"one launch {plan} pose")


def test_refusals_and_zero_rows_write_nothing():
    from genpose_amd import _lib
    from genpose_amd._lib import ptr, stream_ptr
    from genpose_amd.samplers import HeunSampler
    net = _net()
    with pytest.raises(ValueError, match="128"):
        HeunSampler(net, 3, 50, 4, "cuda", tile=128, launches="single")
    with pytest.raises(ValueError, match="launches"):
        HeunSampler(net, 3, 5, 4, "cuda", launches="graph")
    assert HeunSampler(net, 3, 5, 4, "cuda").launches == "chain"  # the default has not moved
    B, K, n = 3, 50, 4
    R = B * K
    L = _lib.lib()
    poison = lambda *s: torch.full(s, -777.0, device="cuda")
    x, d, score, out, traj = poison(R, 9), poison(R, 9), poison(R, 9), poison(R, 9), poison(n, R, 9)
    cvec, tvec, sched, centre = torch.zeros(B, 768, device="cuda"), torch.zeros(n + 1, 768, device="cuda"), torch.zeros(2 * n + 2, 4, device="cuda"), torch.zeros(B, 3, device="cuda")
    good = dict(tile=16, ngroups=1, nb=B, k=K, nsteps=n, denoise=1, net=net.w.ref(), cvec=ptr(cvec), tvec=ptr(tvec), sched=ptr(sched),
                centre=ptr(centre), x=ptr(x), d=ptr(d), score=ptr(score), out=ptr(out), traj=ptr(traj))
    order = ("tile", "ngroups", "nb", "k", "nsteps", "denoise", "net", "cvec", "tvec", "sched", "centre", "x", "d", "score", "out", "traj")
    bad = [dict(tile=128), dict(tile=16 | _lib.PLAN_HEADSPLIT), dict(tile=48), dict(nsteps=0), dict(ngroups=0), dict(k=0), dict(ngroups=2, nb=3, tile=32)]
    bad += [{name: None} for name in ("net", "cvec", "tvec", "sched", "centre", "x", "d", "score", "out")]
    for change in bad:
        a = dict(good, **change)
        assert L.gp_heun_solve_tile(*[a[k_] for k_ in order], stream_ptr()) == -1, change
    # tile 0 where gp_heun_layout's choice is the chain form (a frame of 256 clouds x 50: without a plan of 16 / 32 / 64 rows) is refused too
    t = ctypes.c_int(0)
    if L.gp_heun_layout(0, 1, 640, 50, ctypes.byref(t)) == 0 and t.value == 128:
        assert L.gp_heun_solve_tile(*[dict(good, tile=0, nb=640)[k_] for k_ in order], stream_ptr()) == -1
    assert L.gp_heun_solve_tile(*[dict(good, nb=0)[k_] for k_ in order], stream_ptr()) == 0  # zero rows: GP_OK
    torch.cuda.synchronize()
    for buf in (x, d, score, out, traj):
        assert bool((buf == -777.0).all())
