"""GPU: the fp32 score / energy network kernels against FLOAT64 ground truth (tests/f64_reference.py), on every launch plan.

The fp32 kernels are the default of every tile plan, the only arithmetic of the energy model and of the vector-Jacobian kernels, and the
yardstick in every split-bf16 gate - and were themselves held only to the fp32 CPU oracle at 2e-4 of the scale (NET_RTOL), two to three
orders of magnitude above what they deliver and above the frozen two-term split's error class.

THE RULE.  Per (model, quantity, block, t), E_oracle is the fp32 CPU oracle's own error against float64 - max |fp32 - f64| / max |f64|
per block - maximised over the shape set, both pose scales and the four weight sets (f64_reference.e_oracle_cell; it never sees a kernel
and is computed here, in milliseconds).  A device result passes when its block error <= MARGIN x E_oracle, MARGIN = 3: the allowance for
two fp32 evaluations that round only in their accumulations but in different orders (MFMA k-blocks of 4 in a fixed chain against oneDNN's
blocked sums).  The margin was fixed before any kernel was measured against it; profiles/f64_gate.txt holds every cell of a run (oracle,
device, ratio).  A plan that needs more is an exception NAMED in EXCEPTIONS with its cause, gated at the next power of two above what it
measured and never above MARGIN_CAP = 8: beyond that a result is in the split-bf16 class and is a bug.

THE EXCEPTIONS, one cause.  Every plan consumes cvec, and gp_cloud_embed (csrc/scorenet.hip: cloud_embed_kernel -> mfma_tile) sums the
1024 cloud features of an output in ONE k-ordered fp32 chain of 256 MFMA k-blocks, where the oracle's sgemm spreads the sum over vector
lanes and k-blocks.  The partial sums of such a chain grow like a random walk and every addition rounds at their size: emulated on the host
(one fp32 accumulator, four products per step), the chain is 2.5x to 4.3x the oracle's sgemm on these features (5e-7 to 7e-7 of the block
scale against 2e-7), and the kernel pair measures 3.35x.  That is a property of the accumulation order, not a lost bit: no fast-math
intrinsic, fold or hoist is involved (the epilogues divide by sigma exactly as the reference does).  It crosses 3x only on the ONE-ROW
shape - whose block scale is the largest of three numbers, not of 450 - and at t <= 0.15, where the oracle's own error is smallest; the
86- and 150-row shapes, the 128-row chain forms and every first evaluation at t = 1 stay under 3x.  Measured worst ratios (MI355X):
cloud+time embed 3.35; score_eval tiles 16 / auto 3.85 (score) and 3.02 (energy), tiles 32 / 64 4.003 (score) and 3.64 (energy);
gp_score_div 3.85; gp_energy_score 4.015; Heun's 16-row vector-Jacobian form 3.86.  4.003 and 4.015 fall a hair over 4 and so take the
gate of 8 by the rule, which on those two plans no longer separates the two-term split (the control measures 4.5x to 6.6x): the table
in profiles/f64_gate.txt says so, and the plans' other cells show them in the fp32 class.

Blocks: the three heads of a 9-column output, each column of the 2-column energy, the whole vector for the divergence and the energy of
gp_energy_score.  Derivative quantities (gp_score_div's e^T J e, the energy model's score) are compared on kink-free rows
(f64_reference.kink_free; at most KINK_SHARE of a case, asserted on the host in test_f64_reference_cpu.py and here).

Inputs: shapes (1,1), (3,7), (2,43), (3,50); pose scales 1 and 50; t in {1e-5, 1e-3, 0.15, 0.55, 1}; weights seed 0, seed 1, the stress
state dict of test_gpu_weight_seeds.py and the trained checkpoints.  t = 1 puts arguments of several hundred radians into sinf / cosf,
t = 1e-5 puts them near zero.

POSITIVE CONTROL: the first evaluation of the frozen, opt-in bf16x3 PC step on the 150-row shape must FAIL the rule - a gate that passes
the two-term split is not a gate."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import f64_reference as fr

HS = 0x100  # GP_PLAN_HEADSPLIT
EPS = 1e-5
CHAIN_SHAPES = [(B, K) for B, K in fr.SHAPES if K >= 43]  # the 128-row chain form serves K >= 43
# (family, plan, quantity) -> (gate, cause): plans granted more than MARGIN (module text: one cause, the single accumulation chain of cvec)
CHAIN = "cvec: one k-ordered fp32 chain over 1024 cloud features (gp_cloud_embed); shows on the one-row shape"
EXCEPTIONS = {("cloud+time embed", "-", "embed"): (4.0, CHAIN),
              ("score_eval", "tile=16", "score"): (4.0, CHAIN), ("score_eval", "tile=auto", "score"): (4.0, CHAIN),
              ("score_eval", "tile=32", "score"): (8.0, CHAIN), ("score_eval", "tile=64", "score"): (8.0, CHAIN),
              ("score_eval", "tile=16", "energy"): (4.0, CHAIN), ("score_eval", "tile=auto", "energy"): (4.0, CHAIN),
              ("score_eval", "tile=32", "energy"): (4.0, CHAIN), ("score_eval", "tile=64", "energy"): (4.0, CHAIN),
              ("gp_score_div", "tile", "sdiv"): (4.0, CHAIN), ("gp_energy_score", "tile", "escore"): (8.0, CHAIN),
              ("heun first evaluation", "16 energy vjp", "escore"): (4.0, CHAIN)}

_cache = {}


def _net(which, model):
    from genpose_amd.scorenet import ScoreNetHIP
    if ("net", which, model) not in _cache:
        _cache["net", which, model] = ScoreNetHIP(fr.state_dict(which, model), "cuda")
    return _cache["net", which, model]


def _inputs(which, model, B, K, scale):
    """device copies of the case's inputs and the cloud embedding: -> (cvec, pose, probe, centre)"""
    key = ("in", which, model, B, K, scale)
    if key not in _cache:
        feat, pose, probe, centre = fr.inputs(B, K, scale)
        _cache[key] = (_net(which, model).cloud_embed(feat.cuda()), pose.cuda(), probe.cuda(), centre.cuda())
    return _cache[key]


def _time(net, t):
    """tvec [768] and sigma [1] of the fp32 time the references are given"""
    t32 = float(np.float32(t))
    return net.time_embed(torch.tensor([t32], device="cuda"))[0], torch.tensor([0.01 * 5000.0 ** t32], device="cuda")


def _cell(family, plan, which, quantity, t, shapes, run, beside=None):
    """One (kernel family, plan, weights, quantity, t): run(B, K, scale) -> the device result in the structure of f64_reference.evaluate
    (None for an output the plan does not produce), over `shapes` x pose scales.  Prints oracle / device / ratio per block, returns the
    blocks over their gate.  beside(B, K, scale): a second result printed next to it, not gated."""
    E = fr.e_oracle_cell(quantity, t)
    worst, other, where, dropped = {}, {}, {}, 0.0
    for B, K in shapes:
        for sc in (fr.POSE_SCALES if quantity != "embed" else fr.POSE_SCALES[:1]):
            c = fr.case(which, quantity, B, K, sc, t)
            if c["keep"] is not None:
                dropped = max(dropped, 1.0 - float(c["keep"].double().mean()))
            for store, fn in ((worst, run), (other, beside)):
                if fn is not None:
                    for n, e in fr.errors(fn(B, K, sc), c, quantity).items():
                        old = store.get(n, [0.0] * len(e))
                        if store is worst:
                            where[n] = [(B, K, sc) if b > a else w for a, b, w in zip(old, e, where.get(n, [None] * len(e)))]
                        store[n] = [max(a, b) for a, b in zip(old, e)]
    gate = EXCEPTIONS.get((family, plan, quantity), (fr.MARGIN, None))[0]
    assert fr.MARGIN <= gate <= fr.MARGIN_CAP
    bad = []
    for n, dev in worst.items():
        for j, (eo, ed) in enumerate(zip(E[n], dev)):
            extra = f" | beside {other[n][j]:.2e} ({other[n][j] / eo:.2f}x)" if n in other else ""
            drop = f" | kink rows <= {dropped:.3f}" if n in ("escore", "sdiv_div") else ""
            B, K, sc = where[n][j]
            print(f"f64gate | {family:22s} | {plan:14s} | {which:7s} | {n:10s} b{j} | t {t:<6g} | oracle {eo:.2e} | device {ed:.2e} | ratio {ed / eo:6.3f}"
                  f" | gate {gate:g} | worst at ({B},{K}) x{sc:g}{extra}{drop}")
            assert eo > 0
            if not ed <= gate * eo:
                bad.append((family, plan, which, n, j, t, eo, ed, round(ed / eo, 3)))
    assert dropped <= fr.KINK_SHARE, (which, quantity, t, dropped)
    return bad


@pytest.mark.parametrize("which", fr.WEIGHTS)
def test_evaluate_on_every_plan(which):
    """gp_score_eval_plan, modes score and energy: 16-, 32- and 64-row tiles, the 128-row chain form (K >= 43) and the automatic choice"""
    bad = []
    for mode in ("score", "energy"):
        net = _net(which, mode)
        for tile in (16, 32, 64, 128, 0):
            for t in fr.TIMES:
                tvec, sigma = _time(net, t)

                def run(B, K, sc):
                    cvec, pose, _, _ = _inputs(which, mode, B, K, sc)
                    return net.evaluate(cvec, K, pose, tvec, sigma, mode, tile=tile)
                bad += _cell("score_eval", f"tile={tile or 'auto'}", which, mode, t, CHAIN_SHAPES if tile == 128 else fr.SHAPES, run)
    assert not bad, bad


@pytest.mark.parametrize("which", fr.WEIGHTS)
def test_cloud_and_time_embedding(which):
    """gp_cloud_embed + gp_time_embed alone: cvec[cloud] + tvec, what the rows consume, against float64
    W[:, :1152] . [pts_feat; relu(t_encoder.1(sin, cos))] + b of the three stacked head layers - wherever the kernels keep the biases"""
    bad = []
    net = _net(which, "score")
    for t in fr.TIMES:
        tvec, _ = _time(net, t)
        bad += _cell("cloud+time embed", "-", which, "embed", t, fr.SHAPES, lambda B, K, sc: _inputs(which, "score", B, K, sc)[0] + tvec)
    assert not bad, bad


@pytest.mark.parametrize("which", fr.WEIGHTS)
def test_score_and_divergence(which):
    """gp_score_div: the score and e^T (d score / d x) e against float64 autograd"""
    bad = []
    net = _net(which, "score")
    for t in fr.TIMES:
        tvec, sigma = _time(net, t)

        def run(B, K, sc):
            cvec, pose, probe, _ = _inputs(which, "score", B, K, sc)
            return net.score_and_divergence(cvec, K, pose, probe, tvec, sigma)
        bad += _cell("gp_score_div", "tile", which, "sdiv", t, fr.SHAPES, run)
    assert not bad, bad


@pytest.mark.parametrize("which", fr.WEIGHTS)
def test_energy_models_score(which):
    """gp_energy_score(with_energy=True): the gradient of the inner-product energy, and that energy, against float64 autograd"""
    bad = []
    net = _net(which, "energy")
    for t in fr.TIMES:
        tvec, sigma = _time(net, t)

        def run(B, K, sc):
            cvec, pose, _, _ = _inputs(which, "energy", B, K, sc)
            return net.energy_score(cvec, K, pose, tvec, sigma, with_energy=True)
        bad += _cell("gp_energy_score", "tile", which, "escore", t, fr.SHAPES, run)
    assert not bad, bad


def _first_pc(which, model, B, K, sc, kernel, **kw):
    """the first score evaluation (t = 1) of a PC sampler on the case's inputs, on the plan the keywords ask for"""
    from genpose_amd.samplers import PCSampler
    cvec, pose, _, centre = _inputs(which, model, B, K, sc)
    smp = PCSampler(_net(which, model), B, K, 2, "cuda", use_graph=False, model=model, **kw)
    assert smp.kernel_name == kernel, (smp.kernel_name, kernel)  # the test must not silently measure another plan
    smp.cvec.copy_(cvec), smp.centre.copy_(centre), smp.x.copy_(pose), smp.z1.zero_(), smp.z2.zero_()
    smp.score.fill_(float("nan"))
    smp.launch_step(0)
    torch.cuda.synchronize()
    return smp.score.clone()


def _first_heun(which, model, B, K, sc, T0, kernel, **kw):
    """the first evaluation (t = T0) of a fixed-step Heun solve on the case's inputs"""
    from genpose_amd.samplers import HeunSampler
    cvec, pose, _, centre = _inputs(which, model, B, K, sc)
    smp = HeunSampler(_net(which, model), B, K, 2, "cuda", use_graph=False, model=model, **kw)
    assert smp.kernel_name == kernel, (smp.kernel_name, kernel)
    smp._write_schedule(T0, EPS)
    smp.cvec.copy_(cvec), smp.centre.copy_(centre), smp.x.copy_(pose)
    smp.score.fill_(float("nan"))
    smp.launch_step(0)
    torch.cuda.synchronize()
    return smp.score.clone()


def _as(quantity, score):
    return (score, None) if quantity == "escore" else score


PC_PLANS = [  # (name, model, quantity, shapes, kernel, keywords)
    ("16+headsplit", "score", "score", fr.SHAPES, "pc_step_kernel<16,0,split>", dict(tile=16 | HS)),
    ("128 f32mfma", "score", "score", CHAIN_SHAPES, "pc_step_chain_kernel<2>", dict(tile=128, trunk="f32mfma")),
    ("16 energy vjp", "energy", "escore", fr.SHAPES, "pc_step_kernel<16,energy>", dict(tile=16)),
    ("128 energy vjp", "energy", "escore", CHAIN_SHAPES, "pc_step_chain_kernel<2,energy>", dict(tile=128)),
]
HEUN_PLANS = [
    ("16", "score", "score", fr.SHAPES, "heun_step_kernel<16>", dict(tile=16)),
    ("128 f32mfma", "score", "score", CHAIN_SHAPES, "heun_step_chain_kernel<2>", dict(tile=128, trunk="f32mfma")),
    ("16 energy vjp", "energy", "escore", fr.SHAPES, "heun_step_kernel<16,energy>", dict(tile=16)),
    ("128 energy vjp", "energy", "escore", CHAIN_SHAPES, "heun_step_chain_kernel<2,energy>", dict(tile=128)),
]


@pytest.mark.parametrize("which", fr.WEIGHTS)
def test_plans_reached_through_a_samplers_first_evaluation(which):
    """The head-split plan, the fp32-MFMA chain form and the energy model's vector-Jacobian tile and chain forms: PCSampler's launch 0
    (t = 1), and HeunSampler's from T0 = 0.15 and 0.55, so the chain and vjp forms are also seen away from t = 1.  The bf16x9 trunk on
    the chain plan's rows is printed beside the fp32 figure; its own tests gate it."""
    bad = []
    for name, model, q, shapes, kernel, kw in PC_PLANS:
        beside = None
        if name == "128 f32mfma":
            beside = lambda B, K, sc: _first_pc(which, "score", B, K, sc, "pc_step_chain_kernel<bf16x9>", tile=128, trunk="bf16x9")
        bad += _cell("pc first evaluation", name, which, q, 1.0, shapes, lambda B, K, sc: _as(q, _first_pc(which, model, B, K, sc, kernel, **kw)), beside)
    for name, model, q, shapes, kernel, kw in HEUN_PLANS:
        for T0 in (0.15, 0.55):
            bad += _cell("heun first evaluation", name, which, q, T0, shapes,
                         lambda B, K, sc: _as(q, _first_heun(which, model, B, K, sc, T0, kernel, **kw)))
    assert not bad, bad


@pytest.mark.parametrize("which", fr.WEIGHTS)
def test_positive_control_bf16x3_fails_the_rule(which):
    """The frozen two-term-class split (PCSampler(precision='bf16x3'), opt-in) on the 150-row shape: its first evaluation must exceed
    MARGIN x E_oracle in some head - the very check the fp32 plans pass above."""
    B, K = 3, 50
    over = _cell("pc first evaluation", "bf16x3 CONTROL", which, "score", 1.0, [(B, K)],
                 lambda B, K, sc: _first_pc(which, "score", B, K, sc, "pc_step_bf16x3_kernel", precision="bf16x3"))
    worst = max((b[-1] for b in over), default=0.0)
    print(f"f64gate | positive control, {which}: {len(over)} of 3 heads over {fr.MARGIN:g}x, worst ratio {worst:.3f}")
    assert over, "the bf16x3 trunk passes the fp32 gate: the gate does not separate the arithmetic classes"
