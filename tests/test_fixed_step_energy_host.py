"""CPU (no GPU): the fixed-step solvers on the energy model - the C ABI's `_model` entry points, the opt-in switches (cfg.fixed_step_energy,
sample_from= of both runners, model= of the samplers) with every default and every earlier refusal as it was, and the CONDITIONING of the
inputs tests/test_gpu_fixed_step_energy.py holds the kernels to: the same solve on the CPU oracle with the network evaluated in float32
agrees with the float64 one to a quarter of that file's bound, so the bound cannot be failed by the inputs alone."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import fixed_step_energy_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gp_heun_layout_model", "gp_heun_step_plan_model", "gp_dpm2m_step_plan_model", "gp_heun_solve_tile_model", "gp_dpm2m_solve_tile_model"]
UNSUFFIXED = {name: name[: -len("_model")] for name in NEW_SYMBOLS}


# ------------------------------------------------------------------------------------------------ C ABI
def _prototype(name):
    hdr = open(os.path.join(ROOT, "include", "genpose_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/genpose_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_symbols_are_declared_bound_and_exported(name):
    from genpose_amd import _lib, build
    args = _prototype(name)
    sig = _lib.SIGNATURES[name]
    assert len(sig) == len(args), (name, len(sig), len(args))
    for decl, ct in zip(args, sig):
        want = "pointer" if "*" in decl or decl.startswith("gp_stream_t") else "int"
        assert want == ("int" if ct is ctypes.c_int else "pointer"), (name, decl, ct)
    # a leading `model`, then the unsuffixed entry point's arguments
    assert args[0] == "int model" and args[1:] == _prototype(UNSUFFIXED[name]), name
    build.build()
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), name)


def test_every_prototype_has_its_comment_citing_the_reference():
    hdr = open(os.path.join(ROOT, "include", "genpose_hip.h")).read()
    for name in NEW_SYMBOLS:
        at = hdr.index("int " + name + "(")
        if name == "gp_dpm2m_solve_tile_model":  # declared under the comment it shares with gp_heun_solve_tile_model
            at = hdr.index("int gp_heun_solve_tile_model(")
        before = hdr[:at].rstrip()
        assert before.endswith("*/"), f"{name}: no comment in front of the declaration"
        comment = before[before.rindex("/*"):]
        assert "samplers.py:230-290" in comment and "energynet.py:200-222" in comment, name


def test_model_refusals_need_no_gpu():
    """GP_EINVAL before anything touches a device: model 1 with 32 / 64-row tiles or the head-split plan, a model other than 0 / 1, a
    workgroup straddling two groups, a chain form whose workgroups span too many clouds, model 1 without the transposed weights, the
    one-launch form on plan 128."""
    from genpose_amd import _lib
    L = _lib.lib()
    t = ctypes.c_int(-7)
    for tile in (32, 64, 48, 16 | _lib.PLAN_HEADSPLIT):
        assert L.gp_heun_layout_model(1, tile, 1, 3, 50, ctypes.byref(t)) == -1 and t.value == -7, tile
    assert L.gp_heun_layout_model(2, 16, 1, 3, 50, ctypes.byref(t)) == -1 and L.gp_heun_layout_model(-1, 16, 1, 3, 50, ctypes.byref(t)) == -1
    assert L.gp_heun_layout_model(1, 128, 1, 30, 5, ctypes.byref(t)) == -1  # k = 5: 128 rows span more clouds than the chain form stages
    assert L.gp_heun_layout_model(1, 16, 2, 3, 5, ctypes.byref(t)) == -1  # 15 rows per group: a tile would straddle two groups
    assert L.gp_heun_layout_model(1, 128, 2, 3, 50, ctypes.byref(t)) == -1 and t.value == -7
    assert L.gp_heun_layout_model(1, 16, 1, 3, 5, ctypes.byref(t)) == 0 and t.value == 16
    assert L.gp_heun_layout_model(1, 128, 1, 3, 50, ctypes.byref(t)) == 0 and t.value == 128
    for tile in (16, 32, 64, 128):  # model 0 is gp_heun_layout (tile 0 asks the device for its CU count: tests/test_gpu_fixed_step_energy.py)
        a, b = ctypes.c_int(-1), ctypes.c_int(-1)
        assert L.gp_heun_layout_model(0, tile, 1, 3, 50, ctypes.byref(a)) == L.gp_heun_layout(tile, 1, 3, 50, ctypes.byref(b)) and a.value == b.value
    one = ctypes.c_void_p(16)  # never dereferenced: every call below is refused first
    bare = ctypes.pointer(_lib.GpScoreNet())  # no transposed packs
    good = dict(model=1, tile=16, ngroups=1, nb=3, k=50, launch=1, nsteps=4, denoise=1, net=bare, cvec=one, tvec=one, sched=one, centre=one, x=one, d=one,
                score=one, out=one, traj=one)
    step = ("model", "tile", "ngroups", "nb", "k", "launch", "nsteps", "denoise", "net", "cvec", "tvec", "sched", "centre", "x", "d", "score", "out", "traj")
    solve = tuple(k for k in step if k != "launch")
    bad = [dict(), dict(tile=128), dict(tile=32), dict(tile=64), dict(tile=16 | _lib.PLAN_HEADSPLIT), dict(model=2), dict(model=-1), dict(nsteps=0), dict(k=0)]
    bad += [{name: None} for name in ("net", "cvec", "tvec", "sched", "centre", "x", "d", "score", "out")]
    for change in bad:  # (`dict()`: everything in order but the transposed weights)
        a = dict(good, **change)
        for fn in (L.gp_heun_step_plan_model, L.gp_dpm2m_step_plan_model):
            assert fn(*[a[k] for k in step], None) == -1, change
        for fn in (L.gp_heun_solve_tile_model, L.gp_dpm2m_solve_tile_model):
            assert fn(*[a[k] for k in solve], None) == -1, change
    full = _lib.GpScoreNet(**{n: 16 for n, _ in _lib.GpScoreNet._fields_})
    a = dict(good, net=ctypes.pointer(full), tile=128)
    for fn in (L.gp_heun_solve_tile_model, L.gp_dpm2m_solve_tile_model):
        assert fn(*[a[k] for k in solve], None) == -1  # the chain form keeps its per-launch kernels
    # zero rows: GP_OK, nothing launched
    a = dict(good, net=ctypes.pointer(full), nb=0)
    assert L.gp_heun_step_plan_model(*[a[k] for k in step], None) == 0 and L.gp_dpm2m_solve_tile_model(*[a[k] for k in solve], None) == 0


# ------------------------------------------------------------------------------------------------ the opt-in switches
def _cpu_agent(**kw):
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    return PoseNet(get_config(device="cpu", **kw))


@pytest.mark.parametrize("sampler", ["heun", "dpm2m"])
def test_config_switch_and_both_refusals(sampler):
    from genpose_amd.config import get_config
    assert get_config().fixed_step_energy is False
    off = _cpu_agent(posenet_mode="energy", sampler_mode=[sampler], sampling_steps=8)
    for call in (lambda: off.net.sample({}, sampler), lambda: off.net({}, mode=sampler + "_sample")):
        with pytest.raises(NotImplementedError, match=sampler) as e:
            call()
        assert "fixed_step_energy" in str(e.value) and "posenet_mode='energy'" in str(e.value)
    on = _cpu_agent(posenet_mode="energy", sampler_mode=[sampler], sampling_steps=8, fixed_step_energy=True)
    with pytest.raises(RuntimeError, match="no weights"):  # past the refusal: it fails for lack of weights
        on.net.sample({}, sampler)
    with pytest.raises(ValueError, match="sampling_steps"):
        _cpu_agent(posenet_mode="energy", sampler_mode=[sampler], sampling_steps=None, fixed_step_energy=True).net.sample({}, sampler)
    # the switch means nothing to a score agent
    with pytest.raises(RuntimeError, match="no weights"):
        _cpu_agent(sampler_mode=[sampler], sampling_steps=8, fixed_step_energy=True).net.sample({}, sampler)


def test_single_frame_runner_sample_from():
    from genpose_amd.runner import SingleFrameRunner
    sa, ea = _cpu_agent(), _cpu_agent(posenet_mode="energy")
    assert inspect.signature(SingleFrameRunner.__init__).parameters["sample_from"].default == "score"
    assert SingleFrameRunner(sa, ea).sample_from == "score" and SingleFrameRunner(sa).sample_from == "score"
    one = SingleFrameRunner(None, ea, sample_from="energy")
    assert one.sample_from == "energy" and one.ranker == "energy" and one.score_agent is None
    assert SingleFrameRunner(None, ea, sample_from="energy", ranker="consensus").ranker == "consensus"
    with pytest.raises(ValueError, match="likelihood"):
        SingleFrameRunner(sa, ea, sample_from="energy", ranker="likelihood")
    with pytest.raises(ValueError, match="posenet_mode"):
        SingleFrameRunner(sa, sa, sample_from="energy")  # a score-mode agent cannot be the one network
    with pytest.raises(ValueError, match="energy_agent"):
        SingleFrameRunner(sa, sample_from="energy")
    with pytest.raises(ValueError, match="'score'.*'energy'"):
        SingleFrameRunner(sa, ea, sample_from="both")
    with pytest.raises(NotImplementedError, match="ranker"):  # as before
        SingleFrameRunner(sa, ea, ranker="mean")


def test_fixed_step_tracker_sample_from():
    from genpose_amd.runner import FixedStepTracker
    sa, ea = _cpu_agent(sampler_mode=["heun"], sampling_steps=8), _cpu_agent(posenet_mode="energy")
    assert inspect.signature(FixedStepTracker.__init__).parameters["sample_from"].default == "score"
    assert FixedStepTracker(sa, ea).sample_from == "score"
    with pytest.raises(ValueError, match="posenet_mode"):  # the default keeps the earlier refusal
        FixedStepTracker(ea, ea)
    one = FixedStepTracker(None, ea, sample_from="energy")
    assert one.sample_from == "energy" and one.ranker == "energy" and one.energy_agent is ea and one.score_agent is None
    assert FixedStepTracker(None, ea, sample_from="energy", ranker="consensus", solver="dpm2m").energy_agent is ea
    with pytest.raises(ValueError, match="likelihood"):
        FixedStepTracker(sa, ea, sample_from="energy", ranker="likelihood")
    with pytest.raises(ValueError, match="posenet_mode"):
        FixedStepTracker(sa, sa, sample_from="energy")
    with pytest.raises(ValueError, match="energy_agent"):
        FixedStepTracker(sa, sample_from="energy")
    with pytest.raises(ValueError, match="'score'.*'energy'"):
        FixedStepTracker(sa, ea, sample_from="both")
    with pytest.raises(NotImplementedError, match="pointnet_and_pointnet2"):
        FixedStepTracker(None, _cpu_agent(posenet_mode="energy", pts_encoder="pointnet_and_pointnet2"), sample_from="energy")
    assert one.step([None, None]) == [None, None]  # nothing live: nothing touched
    # launches=None: the score model's small frames take the one-launch solve as before; the energy model's keep the chain (measured slower
    # as one launch, profiles/fixed_step_energy.txt); a forced form is honoured
    assert FixedStepTracker(sa, ea)._solve_form(250, 16) == "single" and one._solve_form(250, 16) == "chain" and one._solve_form(32000, 128) == "chain"
    assert FixedStepTracker(None, ea, sample_from="energy", launches="single")._solve_form(250, 16) == "single"


@pytest.mark.parametrize("cls", ["HeunSampler", "Dpm2mSampler"])
def test_sampler_model_keyword_is_checked_before_the_device(cls):
    from genpose_amd import samplers
    S = getattr(samplers, cls)
    assert inspect.signature(S.__init__).parameters["model"].default == "score" and S.MODELS == ("score", "energy")
    with pytest.raises(ValueError, match="bf16x9"):
        S(None, 3, 5, 4, "cpu", model="energy", trunk="bf16x9")
    with pytest.raises(ValueError, match="'score'.*'energy'"):
        S(None, 3, 5, 4, "cpu", model="likelihood")
    for tile in (32, 64):  # the energy model has plans 16 and 128
        with pytest.raises(ValueError, match="energy model"):
            S(None, 3, 50, 4, "cpu", model="energy", tile=tile)
    with pytest.raises(ValueError, match="128"):
        S(None, 3, 50, 4, "cpu", model="energy", tile=128, launches="single")


# ------------------------------------------------------------------------------------------------ conditioning of the GPU tests' inputs
QUARTER = 0.25


@pytest.mark.parametrize("shape,weights,T0,grid,solver", fc.COMBOS)
def test_float32_network_agrees_with_float64_to_a_quarter_of_the_gpu_bound(shape, weights, T0, grid, solver):
    """The restatement driving go.energy_score with the network in float32 against the same in float64 (the state stays float64 in both:
    what differs is the rounding of the score, which is what the flow amplifies), on every (shape, weights, T0, grid, solver) of the GPU
    file at its N: trajectory, last state and denoised state within a quarter of rtol = atol = 1e-3.  Three of the 36 combinations missed
    it - 0.89, 1.03 and 23.5, one row of 150 each - and are left out here and there by name (fixed_step_energy_cases.DROPPED); nothing is
    widened for them."""
    ref = fc.reference(shape, weights, T0, grid, solver)
    f32 = fc.reference(shape, weights, T0, grid, solver, dtype=torch.float32)
    worst = max(fc.ratio(a, b) for a, b in zip(f32, ref))
    print(f"{shape} {weights} T0={T0} {grid} {solver}: max |f32 - f64| / (atol + rtol |f64|) = {worst:.3e}")
    assert all(bool((abs(a) < 1e30).all()) for a in ref)
    assert worst <= QUARTER, worst
