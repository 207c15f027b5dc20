"""GPU: the fixed-step solvers - HeunSampler, Dpm2mSampler, PCSampler with injected noise - against FLOAT64 solves, held to the fp32 CPU
restatement's own error (tests/solver_reference.py).  This file carries the solvers' accuracy claim; the rtol = atol = 1e-3 of
test_gpu_heun.py, test_gpu_dpm2m.py, test_gpu_fixed_step_energy.py, test_gpu_sched_classes.py and test_gpu_sampler.py stays as a coarse
check (a corrector weight off by 1e-4 passes it at a third of the bound and is 70x or more the oracle's error here).

THE RULE.  Per case, output and block (0:3, 3:6, 6:9), E_oracle is the maximum over R = 8 realisations of the fp32 restatement's block
error against the float64 solve of the unperturbed inputs - realisation 0 is the case's inputs, the others move every element of x0 by one
float32 ulp up or down by a seeded coin (solver_reference.e_oracle; it never sees a kernel).  A device result passes at block_error <=
MARGIN x E_oracle with f64_reference.MARGIN = 3: the solves are recursions of the single evaluations that tests/test_gpu_f64_score.py holds
to that margin.  A plan that needs more is a named exception of EXCEPTIONS with ONE cause shown by a host emulation of the accumulation
order, gated at the next power of two above what it measured and never above MARGIN_CAP = 8; beyond 8 a result is a bug.
profiles/solver_f64_gate.txt holds every cell of a run (oracle, device, ratio).

THE EXCEPTIONS, one cause: the cloud embedding.  Every plan's kernels consume cvec [B,768] = W[:, :1024] . features + bias, and
gp_cloud_embed sums its 1024 terms as ONE k-ordered chain of fp32 fused multiply-adds where the oracle's sgemm spreads the sum over vector
lanes and k-blocks.  The partial sums of such a chain walk at random and every addition rounds at their size; on the trained checkpoints,
whose pre-activations cancel, that is several times the blocked sums' error, it is the same for every row of a cloud and every step of a
solve, and the solve carries it along.  It is the cause tests/test_gpu_f64_score.py names for its own exceptions.  Shown twice:
  - ON THE DEVICE, for every exception (test_the_exceptions_are_the_cloud_embeddings_chain): the same kernels, plans, schedules and
    inputs with cvec formed in float64 on the host and rounded once.  All 23 exceptions then pass at the plain margin of 3 - measured
    0.7x to 2.0x - tile, fp32-MFMA chain and split-bf16 plans, the energy model's vector-Jacobian forms, trained and seeded weights alike.
    Nothing in the step kernels' own arithmetic needs more than 3.
  - ON THE HOST (solver_reference.chain_network, test_solver_reference_cpu.py): the fp32 restatement with the cloud embedding alone
    summed as such a chain is 3.3x to 8.3x E_oracle on the exceptions' shapes, models and weights (15, 21, 69 and 150 rows), chaining
    every other dot product as well changes that by less than a third, and on the worst case the raw state agrees block by block
    (7.6e-7 / 5.4e-7 / 2.7e-6 emulated, 7.2e-7 / 5.1e-7 / 2.5e-6 on the device, 1.7e-7 / 2.1e-7 / 5.9e-7 for the oracle's blocked sums).
    An idealised k-block of four exact products per rounding gives 2.8x there: the roundings per product are what counts.
Sixteen exceptions are the fixed-step plans on the trained checkpoints (3.3x - 7.9x: gates 4 and 8), seven are seeded-weight plans between
3.09x and 4.005x; the other seeded-weight plans reach 2.97x, and every PC plan is 0.9x - 1.3x (its noise and per-step renormalisation do
not let the error accumulate).  At gate 8 the rule no longer separates a two-term split on those plans; the PC control below, the same
plans' cells on an exact cloud embedding at 3, and the seeded-weight cells at 3 do.  A cloud embedding summed in blocks would remove the
exceptions; it would also change the bits of every recorded chain, and is not part of this change.

THE YARDSTICK MOVES WITH THE HOST.  E_oracle is computed by the CPU that runs the test: torch's sgemm blocks and threads its sums by the
machine, and the fp32 restatement's error moves with it (between two CPUs: typically by 1.0x - 1.6x per cell, a spread of 1.31 became 2.27,
and an energy-model case crossed a ReLU kink of the gradient and went from 2.2e-5 to 1.7e-2).  The gates above were measured with the
yardstick of one CPU; the closest cells sit 1 - 2 % under their gate (7.860 of 8; 2.973 of 3), so on another CPU or thread count a cell
can cross its gate, and a case its 2x condition, with no change in the device code.  tests/conftest.py caps the oracle's threads at 16; the
CPU test prints every figure (`solver-oracle |`) so that such a flip can be told from a regression.

Block metric: f64_reference.block_error's max |got - ref| / max |ref| per block.  On finished outputs (trajectory, pose, xs, mean_x) the
cloud-centre rows are first subtracted from the translation block of both sides - a centre of 0.3 would otherwise set the scale at
T0 = 0.15; the raw final state (smp.x) is compared as it is.

CONDITIONS ON THE REFERENCE ALONE (asserted in tests/test_solver_reference_cpu.py, on the host, without a device): a case is admitted only
if every realisation is at most 2x the maximum of the other seven in every output and block; a case that breaks this takes another input
seed (solver_reference.SEEDS, each with the figure of the draw it replaces) or is dropped by name (solver_reference.DROPPED: at most one
case in four of a (solver, model, T0) group; two today); E_oracle stays under solver_reference.ceiling(case).  On the energy model these
conditions decide admission, not fixed_step_energy_cases' quarter-of-1e-3 check: of its three DROPPED combinations one runs here on another
draw and two stay out (a ReLU kink of the gradient that every realisation crosses: spread 1.00, E 1.2e-3 and 1.4e-3 over the ceiling).

Cases.  Heun and DPM-Solver++(2M), score model, N = 6, test_gpu_heun.PLANS (tile16 3x5 = 15 rows; tile32 / tile64 3x23 = 69 rows, tails of
5; chain_f32 / chain_bf16x9 3x50 = 150 rows, a 22-row tail), T0 in {0.15, 0.55, 1}, both grids, denoise both ways, weights seed 0, seed 1
and the trained checkpoint; N = 1 (Heun) and N = 2 (DPM-Solver++(2M): the first step that uses wp and the carried denoiser) on tile16.  The
same two on the energy model over fixed_step_energy_cases.SHAPES x CASES.  PC with injected noise, N = 20: tiles 16 / 32 / 64, the fp32
chain, trunk='bf16x9' and products=6 at 3x50, two batches in one launch once, the energy model on tile 16 and the chain; N = 100 at 3x50
with products=6 (the headline's arithmetic).  The split-bf16 plans get the fp32 bound: that is the project's claim for them.  Every sampler's
kernel_name is asserted, so no case runs another kernel silently.  Every fixed-step run also reads the device's schedule table back and
compares it, bit for bit, with the reference modules' float64 coefficients rounded once - a coefficient formed in float32 moves a solve
by a few hundredths of E_oracle, which no accuracy gate can see.

POSITIVE CONTROL: precision='bf16x3' on the 3x50 PC case must FAIL the rule.

Not repeated here (tied bit for bit to the per-launch chain by existing tests): the one-launch solves, schedule classes, graph replay,
row locality."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dpm2m_reference as dr
import f64_reference as fr
import heun_reference as hr
import solver_reference as sr
import test_gpu_dpm2m as td
import test_gpu_heun as th
from fixed_step_energy_cases import SHAPES as ENERGY_SHAPES
from test_gpu_fixed_step_energy import CHAIN_KERNEL as ENERGY_KERNELS

PLANS = th.PLANS
KERNELS = {"heun": th.KERNELS, "dpm2m": td.KERNELS}
# (family, plan, weights) -> gate: plans granted more than MARGIN, the worst ratio measured on MI355X beside each (module text: one cause)
EXCEPTIONS = {
    ("heun", "tile16", "trained"): 8.0,             # 7.860
    ("heun", "tile32", "trained"): 8.0,             # 6.352
    ("heun", "tile64", "trained"): 8.0,             # 6.352
    ("heun", "chain_f32", "trained"): 8.0,          # 5.327
    ("heun", "chain_bf16x9", "trained"): 8.0,       # 5.488
    ("heun", "tile16", "seed0"): 4.0,               # 3.092 (T0 = 0.15, geometric, finished rotation of x_N; the emulation on this shape: 3.27)
    ("heun", "tile32", "seed0"): 8.0,               # 4.005: a hair over 4, so 8 by the rule
    ("heun", "tile64", "seed0"): 8.0,               # 4.005
    ("heun", "chain_f32", "seed1"): 4.0,            # 3.529
    ("heun", "chain_bf16x9", "seed1"): 4.0,         # 3.583
    ("dpm2m", "tile16", "trained"): 8.0,            # 7.254
    ("dpm2m", "tile32", "trained"): 8.0,            # 5.937
    ("dpm2m", "tile64", "trained"): 8.0,            # 5.937
    ("dpm2m", "chain_f32", "trained"): 8.0,         # 4.967
    ("dpm2m", "chain_bf16x9", "trained"): 8.0,      # 4.560
    ("dpm2m", "chain_bf16x9", "seed1"): 4.0,        # 3.377
    ("heun energy", "tile16", "trained"): 4.0,      # 3.615
    ("heun energy", "tile16x2", "trained"): 8.0,    # 5.322
    ("heun energy", "chain", "trained"): 8.0,       # 6.020
    ("dpm2m energy", "tile16", "trained"): 4.0,     # 3.256
    ("dpm2m energy", "tile16x2", "trained"): 8.0,   # 5.188
    ("dpm2m energy", "chain", "trained"): 8.0,      # 5.838
    ("dpm2m energy", "chain", "seed0"): 4.0,        # 3.244
}


@functools.lru_cache(maxsize=None)
def _net(weights, model):
    from genpose_amd.scorenet import ScoreNetHIP
    return ScoreNetHIP(fr.state_dict(weights, model), "cuda")


@functools.lru_cache(maxsize=None)
def _device_inputs(case, exact_cvec=False):
    """exact_cvec: the cloud embedding gp_cloud_embed computes (W[:, :1024] . features + the heads' first-layer bias) formed in float64 on
    the host and rounded once, in place of the kernel's - the one substitution of test_the_exceptions_are_the_cloud_embeddings_chain"""
    feat, centre, x0 = sr.inputs(case)
    cvec = _net(case.weights, case.model).cloud_embed(feat.cuda())
    if exact_cvec:
        sd = fr.state_dict64(case.weights, case.model)
        W = torch.cat([sd[f"{fr.P}fusion_tail_{h}.0.weight"] for h in fr.HEADS], 0)
        b = torch.cat([sd[f"{fr.P}fusion_tail_{h}.0.bias"] for h in fr.HEADS], 0)
        exact = feat.double() @ W[:, :1024].T + b
        assert fr.block_error(cvec, exact, None)[0] < 1e-5  # (the same quantity: the kernel's is an fp32 rounding of it)
        cvec = exact.float().cuda()
    return cvec, centre.cuda(), x0.cuda()


def _gate(family, plan, case, got, gate=None):
    """Prints every cell of `got` ({output: device array}) against the case's float64 solve and returns the cells over their gate."""
    gate = EXCEPTIONS.get((family, plan, case.weights), fr.MARGIN) if gate is None else gate
    assert fr.MARGIN <= gate <= fr.MARGIN_CAP
    E = sr.e_oracle(case)
    err = sr.errors({n: v.detach().cpu().numpy() for n, v in got.items()}, sr.reference(case), case)
    bad = []
    for n, e in err.items():
        for j, (eo, ed) in enumerate(zip(E[n], e)):
            print(f"f64gate | {family:12s} | {plan:14s} | {case.weights:7s} | {case.B}x{case.K} N={case.n:<3d} seed {case.seed} | T0 {case.T0:<4g} {str(case.grid):9s} | "
                  f"{n:6s} b{j} | oracle {eo:.2e} | device {ed:.2e} | ratio {ed / eo:7.3f} | gate {gate:g}")
            assert 0 < eo < sr.ceiling(case)
            if not ed <= gate * eo:
                bad.append((family, plan, tuple(case), n, j, eo, ed, round(ed / eo, 3)))
    return bad


def _check_table(smp, case, denoise):
    """the device's schedule table is the reference modules' float64 coefficients rounded once, bit for bit"""
    N, f = case.n, np.float32
    t, sig, h = hr.grid(N, case.T0, kind=case.grid)
    assert np.array_equal(smp.t_dev.cpu().numpy(), t.astype(f))
    if case.solver == "heun":
        s = smp.sched.cpu().numpy().reshape(-1, 4)
        for first, slope in ((1, -sig[:-1]), (2, -sig[1:])):
            rows = s[first:2 * N + 1:2]
            assert np.array_equal(rows[:, 0], sig[1:].astype(f)) and np.array_equal(rows[:, 1], slope.astype(f)) and np.array_equal(rows[:, 2], h.astype(f))
        last = s[2 * N + 1] if denoise else None
    else:
        s = smp.sched.cpu().numpy().reshape(-1, 8)
        for col, want in zip((1, 2, 4, 5), dr.coefficients(sig)):
            assert np.array_equal(s[1:N + 1, col], want.astype(f)), col
        assert np.array_equal(s[1:N + 1, 0], sig[1:].astype(f))
        last = s[N + 1] if denoise else None
    assert s[0, 0] == f(sig[0])
    if denoise:  # g(eps) is formed in float32 from the rounded sigma (two roundings), the predictor's step rounded once
        assert last[0] == f(sig[N]) and abs(float(last[1]) / (hr.sigma(hr.EPS) * hr.G_FACTOR) - 1.0) < 2e-7 and last[2] == f((1.0 - hr.EPS) / N)


def _fixed_step(case, family, plan, tile, trunk, kernel, denoise, exact_cvec=False):
    from genpose_amd.samplers import Dpm2mSampler, HeunSampler
    cls = HeunSampler if case.solver == "heun" else Dpm2mSampler
    smp = cls(_net(case.weights, case.model), case.B, case.K, case.n, "cuda", tile=tile, trunk=trunk, grid=case.grid, denoise=denoise, record_traj=True,
              model=case.model)
    assert smp.kernel_name == kernel and smp.tile == tile, (smp.kernel_name, kernel)  # the test must not silently measure another plan
    cvec, centre, x0 = _device_inputs(case, exact_cvec)
    xs, pose = smp.run(cvec, centre, x0, T0=case.T0)
    torch.cuda.synchronize()
    assert smp.last_stats["kernel_name"] == kernel and tuple(xs.shape) == (case.B * case.K, case.n, 9) and xs.dtype == pose.dtype == torch.float32
    got = {"traj": xs.permute(1, 0, 2), ("pose" if denoise else "last"): pose, "x": smp.x}
    if exact_cvec:  # (every exception's cells at the plain margin; the table was checked by the plain run)
        return _gate(family + " xcvec", plan, case, got, gate=fr.MARGIN)
    bad = _gate(family, plan, case, got)
    try:
        _check_table(smp, case, denoise)
    except AssertionError as e:
        print(f"f64gate | {family:12s} | {plan:14s} | {case.weights:7s} | T0 {case.T0:<4g} {str(case.grid):9s} | the device's schedule table is not the float64 coefficients rounded once")
        bad.append((family, plan, tuple(case), "schedule table", str(e).splitlines()[0] if str(e) else "mismatch"))
    return bad


@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("T0", sr.T0S)
@pytest.mark.parametrize("weights", sr.SCORE_WEIGHTS)
@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("solver", ["heun", "dpm2m"])
def test_fixed_step_score_model(solver, plan, weights, T0, denoise):
    B, K, tile, trunk = PLANS[plan]
    bad = []
    for grid in sr.GRIDS:
        case = sr.make_case(solver, "score", weights, B, K, T0, grid, sr.N_STEPS)
        bad += _fixed_step(case, solver, plan, tile, trunk, KERNELS[solver][plan], denoise)
    assert not bad, bad


@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("case", sr.SHORT_CASES, ids=lambda c: f"{c.solver}-N{c.n}")
def test_fixed_step_one_and_two_steps(case, denoise):
    B, K, tile, trunk = PLANS["tile16"]
    assert (case.B, case.K) == (B, K)
    bad = _fixed_step(case, case.solver, "tile16", tile, trunk, KERNELS[case.solver]["tile16"], denoise)
    assert not bad, bad


@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("weights,T0", sr.ENERGY_CASES)
@pytest.mark.parametrize("shape", list(ENERGY_SHAPES))
@pytest.mark.parametrize("solver", ["heun", "dpm2m"])
def test_fixed_step_energy_model(solver, shape, weights, T0, denoise):
    B, K, tile = ENERGY_SHAPES[shape]
    bad = []
    for grid in sr.GRIDS:
        case = sr.make_case(solver, "energy", weights, B, K, T0, grid, sr.N_STEPS)
        if case in sr.DROPPED:
            print(f"f64gate | {solver} energy | {shape} | dropped by the conditions on the reference: {sr.DROPPED[case]}")
            continue
        bad += _fixed_step(case, solver + " energy", shape, tile, None, ENERGY_KERNELS[solver, tile], denoise)
    assert not bad, bad


@pytest.mark.parametrize("family,plan,weights", list(EXCEPTIONS), ids=lambda v: str(v).replace(" ", "_"))
def test_the_exceptions_are_the_cloud_embeddings_chain(family, plan, weights):
    """THE CAUSE, PLAN BY PLAN, ON THE DEVICE.  Every case of every named exception once more with ONE thing changed: the cloud embedding
    cvec [B,768], which every plan's kernels consume and gp_cloud_embed sums as one k-ordered fp32 chain over the 1024 cloud features, is
    formed in float64 on the host and rounded once.  The step kernels, their MFMA or split-bf16 arithmetic, the schedule and the inputs are
    the exception's own.  Every cell must then pass at the plain MARGIN = 3: what the exception is granted for is that one chain, on
    this plan's shape and arithmetic, and nothing else in it."""
    solver, model = family.split()[0], ("energy" if family.endswith("energy") else "score")
    bad = []
    for T0 in ((0.15, 0.55, 1.0) if model == "score" else sorted({t for w, t in sr.ENERGY_CASES if w == weights})):
        for grid in sr.GRIDS:
            for denoise in (True, False):
                if model == "score":
                    B, K, tile, trunk = PLANS[plan]
                    case, kernel = sr.make_case(solver, "score", weights, B, K, T0, grid, sr.N_STEPS), KERNELS[solver][plan]
                else:
                    B, K, tile = ENERGY_SHAPES[plan]
                    trunk, case, kernel = None, sr.make_case(solver, "energy", weights, B, K, T0, grid, sr.N_STEPS), ENERGY_KERNELS[solver, tile]
                if case not in sr.DROPPED:
                    bad += _fixed_step(case, family, plan, tile, trunk, kernel, denoise, exact_cvec=True)
    assert not bad, bad


# name -> (case, kernel, PCSampler keywords)
PC_PLANS = {
    "tile16": ("score 3x5", "pc_step_kernel<16>", dict(tile=16)),
    "tile32": ("score 3x23", "pc_step_kernel<32>", dict(tile=32)),
    "tile64": ("score 3x23", "pc_step_kernel<64>", dict(tile=64)),
    "chain_f32": ("score 3x50", "pc_step_chain_kernel<2>", dict(tile=128, trunk="f32mfma")),
    "chain_bf16x9": ("score 3x50", "pc_step_chain_kernel<bf16x9>", dict(tile=128, trunk="bf16x9")),
    "chain_bf16x6": ("score 3x50", "pc_step_chain_kernel<bf16x9,6>", dict(tile=128, trunk="bf16x9", products=6)),
    "tile16 groups=2": ("score 2x(2x8)", "pc_step_kernel<16>", dict(tile=16)),
    "tile16 energy": ("energy 3x5", "pc_step_kernel<16,energy>", dict(tile=16)),
    "chain energy": ("energy 3x50", "pc_step_chain_kernel<2,energy>", dict(tile=128)),
    "chain_bf16x6 N=100": ("score 3x50 N=100", "pc_step_chain_kernel<bf16x9,6>", dict(tile=128, trunk="bf16x9", products=6)),
}


def _pc(name, case, kernel, kw):
    from genpose_amd.samplers import PCSampler
    smp = PCSampler(_net(case.weights, case.model), case.B, case.K, case.n, "cuda", record_traj=True, groups=case.groups, model=case.model, **kw)
    assert smp.kernel_name == kernel, (smp.kernel_name, kernel)
    cvec, centre, x0 = _device_inputs(case)
    z1, z2 = sr.pc_noise(case)
    xs, mean_x = smp.run(cvec, centre, x0, z1.cuda(), z2.cuda())
    torch.cuda.synchronize()
    assert tuple(xs.shape) == (case.B * case.K, case.n, 9) and xs.dtype == mean_x.dtype == torch.float32
    return _gate("pc", name, case, {"xs": xs, "mean_x": mean_x})


@pytest.mark.parametrize("name", list(PC_PLANS))
def test_pc_with_injected_noise(name):
    key, kernel, kw = PC_PLANS[name]
    bad = _pc(name, sr.PC_CASES[key], kernel, kw)
    assert not bad, bad


def test_positive_control_bf16x3_fails_the_rule():
    """The frozen two-term-class split (PCSampler(precision='bf16x3'), opt-in) on the 3x50 PC case: the very check the fp32 and
    exact-product plans pass above."""
    over = _pc("bf16x3 CONTROL", sr.PC_CASES["score 3x50"], "pc_step_bf16x3_kernel", dict(precision="bf16x3"))
    print(f"f64gate | positive control: {len(over)} of 6 cells over {fr.MARGIN:g}x, worst ratio {max((b[-1] for b in over), default=0.0):.3f}")
    assert over, "the bf16x3 trunk passes the solvers' gate: the gate does not separate the arithmetic classes"
