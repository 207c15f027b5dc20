"""CPU (no GPU): the C ABI of the one-launch Heun solve and the tracker's prior (gp_heun_solve_tile, gp_track_warm_start,
gp_track_prior_fill), the prior's counter layout against the PC draws' (tests/track_prior_reference.py), FixedStepTracker's refusals at
construction, and TrackingRunner's two refusals, which stay."""
import ctypes
import os
import re

import numpy as np
import pytest

import philox_reference as pr
import track_prior_reference as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gp_heun_solve_tile", "gp_track_warm_start", "gp_track_prior_fill"]


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
        want = "pointer" if "*" in decl or decl.startswith("gp_stream_t") else "int64" if decl.startswith("int64_t") else "int"
        assert want == ("int" if ct is ctypes.c_int else "int64" if ct is ctypes.c_int64 else "pointer"), (name, decl, ct)
    build.build()
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), name)


def test_prototypes_and_the_reference_lines_they_cite():
    hdr = open(os.path.join(ROOT, "include", "genpose_hip.h")).read()
    solve, step = _prototype("gp_heun_solve_tile"), _prototype("gp_heun_step_plan")
    assert solve == [a for a in step if a != "int launch"]  # the chain's buffers, no launch index
    assert _prototype("gp_track_warm_start") == ["int n", "int k", "const void *seed_state", "const float *sigma", "const float *prev_sRT", "const int *src",
                                                 "const float *fallback_sRT", "const float *centre", "float *x0", "gp_stream_t s"]
    assert _prototype("gp_track_prior_fill") == ["const void *seed_state", "int64_t row0", "int64_t nrows", "float *z_out", "gp_stream_t s"]
    for name, cites in (("gp_heun_solve_tile", ["samplers.py:230-290"]), ("gp_track_warm_start", ["evaluation_tracking.py:262-337", "samplers.py:180"])):
        at = hdr.index("int " + name + "(")
        comment = hdr[hdr.rindex("/*", 0, at):at]
        for c in cites:
            assert c in comment, (name, c)


def test_host_refusals_of_the_entry_points_need_no_device():
    from genpose_amd import _lib
    L = _lib.lib()
    assert L.gp_heun_solve_tile(16, 1, 3, 5, 4, 1, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert L.gp_track_warm_start(3, 4, None, None, None, None, None, None, None, None) == -1
    assert L.gp_track_prior_fill(None, 0, 4, None, None) == -1


def test_the_priors_counters_are_shared_with_no_pc_draw():
    """The prior's step field is 2^29 - 1; a seeded PC sampler takes nsteps < 2^29, so its steps end at 2^29 - 2.  For the same seeds, runs
    and rows, the (counter, key) sets of the prior and of PC draws - both streams, every block, steps up to the last one - are disjoint,
    and the layout's inverse gives the fields back."""
    assert tp.PRIOR_STEP == (1 << 29) - 1
    rng = np.random.default_rng(5)
    seeds = [0, 1, 0xC0FFEE1234567890]
    rows = np.concatenate([tp.global_rows(s, 8, 50) for s in (0, 1, 127)] + [np.array([(1 << 40) + 3, (1 << 64) - 1], dtype=np.uint64)])
    prior, pc = set(), set()
    for seed in seeds:
        for frame in (0, 1, 29, (1 << 32) - 1):
            ctr, key = tp.counters(seed, frame, rows)
            sd, run, step, stream, block, row = pr.unpack(ctr, key)
            assert (sd == np.uint64(seed)).all() and (run == frame).all() and (step == tp.PRIOR_STEP).all() and (stream == 0).all()
            assert (block == np.arange(3, dtype=np.uint64)).all() and (row == rows[:, None]).all()
            prior |= {tuple(w) for w in np.concatenate([ctr, key], axis=-1).reshape(-1, 6).tolist()}
            steps = np.concatenate([np.arange(0, 4), rng.integers(0, tp.PRIOR_STEP, 8), [tp.PRIOR_STEP - 2, tp.PRIOR_STEP - 1]]).astype(np.uint64)
            assert (steps < tp.PRIOR_STEP).all()
            for stream_ in (pr.STREAM_LANGEVIN, pr.STREAM_PREDICTOR):
                for b in range(3):
                    c2, k2 = pr.pack(seed, frame, steps[:, None], stream_, b, rows[None, :])
                    pc |= {tuple(w) for w in np.concatenate([c2, k2], axis=-1).reshape(-1, 6).tolist()}
    assert len(prior) == len(seeds) * 4 * len(rows) * 3  # every prior tuple is its own (counter, key)
    assert not prior & pc
    # the normals are the restatement's generator on those counters
    z = tp.normals(7, 3, tp.global_rows(2, 4, 10))
    assert z.shape == (40, 9) and z.dtype == np.float32 and np.isfinite(z).all() and np.abs(z).max() <= pr.Z_MAX * (1 + 1e-6)
    assert np.array_equal(z, pr.normals(7, 3, tp.PRIOR_STEP, 0, np.uint64(2 * 8 * 10) + np.arange(40, dtype=np.uint64)))


def _cpu_agent(**kw):
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    return PoseNet(get_config(device="cpu", **kw))


def test_constructor_refusals_name_the_option():
    from genpose_amd.runner import FixedStepTracker
    sa, ea = _cpu_agent(sampler_mode=["heun"], sampling_steps=8), _cpu_agent(posenet_mode="energy")
    tr = FixedStepTracker(sa, ea)
    assert (tr.steps, tr.repeat_num, tr.T0, tr.ratio, tr.ranker, tr.launches, tr.grid, tr.max_objects) == (8, 50, 0.15, 0.6, "energy", None, "geometric", 8)
    assert FixedStepTracker(sa, ranker="likelihood").energy_agent is None  # a score checkpoint alone
    with pytest.raises(ValueError, match="posenet_mode"):
        FixedStepTracker(ea, ea)
    with pytest.raises(ValueError, match="energy_agent"):
        FixedStepTracker(sa, ranker="energy")
    with pytest.raises(ValueError, match="ranker"):
        FixedStepTracker(sa, ea, ranker="mean")
    with pytest.raises(NotImplementedError, match="pointnet_and_pointnet2"):
        FixedStepTracker(_cpu_agent(pts_encoder="pointnet_and_pointnet2"), ea)
    with pytest.raises(NotImplementedError, match="pointnet_and_pointnet2"):
        FixedStepTracker(sa, _cpu_agent(posenet_mode="energy", pts_encoder="pointnet_and_pointnet2"))
    coupled = _cpu_agent()
    coupled.net.coupling_group = object()
    with pytest.raises(ValueError, match="coupling_group"):
        FixedStepTracker(coupled, ea)
    with pytest.raises(ValueError, match="steps"):
        FixedStepTracker(sa, ea, steps=0)
    with pytest.raises(ValueError, match="launches"):
        FixedStepTracker(sa, ea, launches="graph")
    with pytest.raises(ValueError, match="grid"):
        FixedStepTracker(sa, ea, grid="cosine")
    assert FixedStepTracker.SINGLE_MAX_ROWS >= 0 and FixedStepTracker.MAX_SHAPES == 8
    assert tr.step([None, None]) == [None, None]  # nothing live: nothing touched


def test_the_tracking_runners_refusals_stay():
    from genpose_amd.runner import TrackingRunner
    sa, ea = _cpu_agent(sampler_mode=["heun"], sampling_steps=8), _cpu_agent(posenet_mode="energy")
    with pytest.raises(NotImplementedError, match="heun"):
        TrackingRunner(sa, ea, use_graphs=True)
    with pytest.raises(NotImplementedError, match="likelihood"):
        TrackingRunner(sa, ea, ranker="likelihood")
    TrackingRunner(sa, ea, use_graphs=False)


def test_sampler_keyword_is_checked_before_the_device():
    from genpose_amd.samplers import HeunSampler
    assert HeunSampler.LAUNCHES == ("chain", "single")
    with pytest.raises(ValueError, match="launches"):
        HeunSampler(None, 3, 5, 4, "cpu", launches="graph")
