"""CPU (no GPU): schedule classes on the fixed-step solvers - the C ABI of gp_heun_step_classes, gp_dpm2m_step_classes, gp_heun_solve_classes,
gp_dpm2m_solve_classes and gp_track_start_classes (declared with the reference lines they generalise, bound, exported; their refusals need
no device), the C-class schedule block of samplers.HeunSampler / Dpm2mSampler(classes=C) against the per-class schedules, and the
constructors' refusals, which name the option."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVE_SYMBOLS = ["gp_heun_step_classes", "gp_dpm2m_step_classes", "gp_heun_solve_classes", "gp_dpm2m_solve_classes"]
NEW_SYMBOLS = SOLVE_SYMBOLS + ["gp_track_start_classes"]


def _header():
    return open(os.path.join(ROOT, "include", "genpose_hip.h")).read()


def _prototype(name):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
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
    build.build()
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), name)


def test_prototypes_are_the_twins_plus_the_classes_and_cite_the_reference():
    hdr = _header()
    tail = ["int ncls", "const int *cls", "gp_stream_t s"]
    for mine, twin in zip(SOLVE_SYMBOLS, ("gp_heun_step_plan_model", "gp_dpm2m_step_plan_model", "gp_heun_solve_tile_model", "gp_dpm2m_solve_tile_model")):
        assert _prototype(mine) == _prototype(twin)[:-1] + tail, mine
    assert _prototype("gp_track_start_classes") == ["int n", "int k", "const void *seed_state", "const float *sched", "int class_stride",
                                                    "const float *prev_sRT", "const int *src", "const float *fallback_sRT", "const float *centre",
                                                    "float *x0", "int *cls_out", "int acquire", "gp_stream_t s"]
    for name, cites in [(n, ["samplers.py:230-290", ":209-218"]) for n in SOLVE_SYMBOLS] + [("gp_track_start_classes", ["samplers.py:180", "evaluation_tracking.py:302-310"])]:
        at = hdr.index("int " + name + "(")
        assert hdr[:at].rstrip().endswith("*/"), f"{name}: no comment in front of the declaration"
        comment = hdr[hdr.rindex("/*", 0, at):at]
        for c in cites:
            assert c in comment, (name, c)
    assert re.search(r"#define\s+GP_MAX_SCHED_CLASSES\s+8\b", hdr)


def test_refusals_of_the_entry_points_need_no_device():
    """GP_EINVAL before anything touches a device: ncls 0 / 9, a null cls, plan 128 (forced), the head-split plan, model 1 - each the only
    thing wrong with the call - and what the twins refuse."""
    from genpose_amd import _lib
    from genpose_amd.samplers import HeunSampler
    L = _lib.lib()
    assert HeunSampler.MAX_CLASSES == 8
    one = ctypes.c_void_p(16)  # never dereferenced: every call below is refused first
    net = ctypes.pointer(_lib.GpScoreNet())
    good = dict(model=0, tile=16, ngroups=1, nb=3, k=50, launch=1, nsteps=4, denoise=1, net=net, cvec=one, tvec=one, sched=one, centre=one, x=one, d=one,
                score=one, out=one, traj=one, ncls=2, cls=one)
    step = ("model", "tile", "ngroups", "nb", "k", "launch", "nsteps", "denoise", "net", "cvec", "tvec", "sched", "centre", "x", "d", "score", "out", "traj",
            "ncls", "cls")
    solve = tuple(k for k in step if k != "launch")
    bad = [dict(ncls=0), dict(ncls=9), dict(ncls=-1), dict(cls=None), dict(tile=128), dict(tile=16 | _lib.PLAN_HEADSPLIT), dict(model=1), dict(model=2),
           dict(tile=48), dict(nsteps=0), dict(ngroups=0), dict(k=0), dict(ngroups=2, nb=3, tile=32)]
    bad += [{name: None} for name in ("net", "cvec", "tvec", "sched", "centre", "x", "d", "score", "out")]
    for change in bad:
        a = dict(good, **change)
        for fn in (L.gp_heun_step_classes, L.gp_dpm2m_step_classes):
            assert fn(*[a[k] for k in step], None) == -1, change
        for fn in (L.gp_heun_solve_classes, L.gp_dpm2m_solve_classes):
            assert fn(*[a[k] for k in solve], None) == -1, change
    for change in (dict(launch=-1), dict(launch=10)):
        assert L.gp_heun_step_classes(*[dict(good, **change)[k] for k in step], None) == -1, change
    # the start kernel: null pointers (the fallback only outside acquire mode), k <= 0, no class stride
    s_good = [3, 4, one, one, 40, one, one, one, one, one, one, 1]
    for i, v in [(0, -1), (1, 0), (4, 0)] + [(j, None) for j in (2, 3, 5, 6, 8, 9, 10)]:
        a = list(s_good)
        a[i] = v
        assert L.gp_track_start_classes(*a, None) == -1, (i, v)
    a = list(s_good)
    a[7], a[11] = None, 0  # no fallback pose and no acquire mode: nothing to start such a cloud from
    assert L.gp_track_start_classes(*a, None) == -1
    a[0] = 0  # zero rows with a null fallback in acquire mode: GP_OK, nothing launched
    a[11] = 1
    assert L.gp_track_start_classes(*a, None) == 0


@pytest.mark.parametrize("solver", ["heun", "dpm2m"])
@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("grid", ["geometric", "edm"])
def test_the_class_block_is_the_per_class_schedules_stacked(solver, denoise, grid):
    from genpose_amd import samplers
    cls_, one = (samplers.Dpm2mSampler, samplers.dpm2m_schedule) if solver == "dpm2m" else (samplers.HeunSampler, samplers.heun_schedule)
    T0s, eps, N = (0.15, 0.55, 1.0), 1e-5, 6
    smp = cls_.__new__(cls_)  # the schedule is host arithmetic: no device, no buffers
    smp.n, smp.grid, smp.rho, smp.denoise = N, grid, 7.0, denoise
    t, sched = smp._class_schedules(T0s, eps)
    L = cls_._launches(N, denoise)
    assert t.shape == (3, N + 1) and t.dtype == np.float64 and sched.shape == (3, L, cls_.SCHED_ROW) and sched.dtype == np.float32
    for c, T0 in enumerate(T0s):
        tc, sc = one(N, T0, eps, grid, 7.0, denoise)
        assert np.array_equal(t[c], tc) and np.array_equal(sched[c], sc), (c, T0)
    # what the kernels read from class 0 is the same in every class: the kind column, and DPM-Solver++(2M)'s first-step mark
    assert (sched[:, :, 3] == sched[0, :, 3]).all()
    if solver == "dpm2m":
        assert ((sched[:, :, 5] != 0) == (sched[0, :, 5] != 0)).all()
    assert not np.array_equal(sched[0, :, 0], sched[1, :, 0])  # (the classes do differ)


def _cpu_agent(**kw):
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    return PoseNet(get_config(device="cpu", **kw))


def test_constructor_refusals_name_the_option():
    from genpose_amd.runner import FixedStepTracker
    from genpose_amd.samplers import Dpm2mSampler, HeunSampler
    for S in (HeunSampler, Dpm2mSampler):
        with pytest.raises(ValueError, match="model"):
            S(None, 3, 5, 4, "cpu", classes=2, model="energy")
        with pytest.raises(ValueError, match="trunk"):
            S(None, 3, 5, 4, "cpu", classes=2, trunk="bf16x9")
        with pytest.raises(ValueError, match="tile"):
            S(None, 3, 50, 4, "cpu", classes=2, tile=128)
        for c in (0, 9):
            with pytest.raises(ValueError, match="classes"):
                S(None, 3, 5, 4, "cpu", classes=c)
    sa, ea = _cpu_agent(sampler_mode=["heun"], sampling_steps=8), _cpu_agent(posenet_mode="energy")
    tr = FixedStepTracker(sa, ea)
    assert (tr.init, tr.acquire_T0) == ("gt", 0.55)  # the default has not moved; acquire_T0 is SingleFrameRunner's T0
    tr = FixedStepTracker(sa, ea, init="prior", acquire_T0=1.0)
    assert (tr.init, tr.acquire_T0) == ("prior", 1.0)
    with pytest.raises(ValueError, match="init"):
        FixedStepTracker(sa, ea, init="bogus")
    with pytest.raises(ValueError, match="sample_from"):
        FixedStepTracker(None, ea, init="prior", sample_from="energy")
    with pytest.raises(ValueError, match="acquire_T0"):
        FixedStepTracker(sa, ea, init="prior", acquire_T0=0.0)
    assert tr.step([None]) == [None]
