"""CPU (no GPU): the C-ABI library loads and exports every symbol include/genpose_hip.h declares; host-side logic
(weight packing, BN folding, schedules, rotations, runner glue, config, error behaviour without a device)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import genpose_oracle as go
from oracle import rot as orot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "genpose_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(gp_[a-z0-9_]+)\s*\(", hdr)))


def test_library_exports_every_declared_symbol():
    from genpose_amd import _lib, build
    build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    syms = declared_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/genpose_hip.h but not exported"
    for s in _lib.SIGNATURES:
        assert s in syms, f"{s} bound in _lib.py but not declared in the header"
    assert _lib.lib().gp_version() == 1


def test_arithmetic_convention_defaults_agree():
    """ONE default for the contraction convention of the three-product sums (include/genpose_hip.h GP_ARITH_*): the header's macro, what
    the built library reports, the Python config the encoder / operator module read, and the oracle's - a flip has to move all four."""
    from genpose_amd import _lib, config
    from oracle import pn2_oracle as ops
    import genpose_amd.pointnet2_cuda as m
    hdr = open(os.path.join(ROOT, "include", "genpose_hip.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"#define GP_ARITH_([ABC]) (\d)", hdr)}
    assert codes == config.DIST_ARITH_CODES == ops.ARITH_CODES
    default_macro = re.search(r"#define GP_ARITH_DEFAULT GP_ARITH_([ABC])", hdr).group(1)
    assert default_macro == config.DEFAULT_DIST_ARITH == ops.DEFAULT_ARITH == m.ARITH == config.get_config().dist_arith
    assert _lib.lib().gp_arith_default() == codes[default_macro]
    with pytest.raises(ValueError):
        config.dist_arith_code("D")
    with pytest.raises(ValueError):
        m.set_arith("fast")
    from genpose_amd.encoder import Pointnet2EncoderHIP
    sd = go.make_state_dict(0, "score")
    encs = {a: Pointnet2EncoderHIP(sd, "cpu", arith=a) for a in "ABC"}
    assert [encs[a].arith for a in "ABC"] == [0, 1, 2]
    # a grouping computed under one convention is not handed to an encoder that runs another
    assert len({encs[a].grouping_key() for a in "ABC"}) == 3
    assert Pointnet2EncoderHIP(sd, "cpu").grouping_key() == encs[config.DEFAULT_DIST_ARITH].grouping_key()
    # bad convention at the C boundary: GP_EINVAL, no launch
    assert _lib.lib().gp_furthest_point_sampling_arith(7, 1, 8, 2, None, None, None, None) == -1
    assert _lib.lib().gp_ball_query_msg_arith(-1, 1, 8, 2, 0.1, 4, 0.2, 4, None, None, None, None, None) == -1


def test_ball_query_msg_fits_is_declared_bound_and_owns_the_limit():
    """gp_ball_query_msg_fits (host only: no device): the header's arity in _lib.SIGNATURES, and the limit the header documents -
    12 n + 16 (nsample0 + nsample1 + 2) bytes within 60 KiB - at its edge for the encoder's neighbourhood sizes.  The fused entry
    refuses exactly what it says does not fit (before it looks at the device)."""
    from genpose_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "genpose_hip.h")).read(), flags=re.S)
    args = re.search(r"\bint\s+gp_ball_query_msg_fits\s*\(([^)]*)\)\s*;", hdr).group(1).split(",")
    assert len(args) == 3 and all(a.split()[0] == "int" and "*" not in a for a in args)
    assert _lib.SIGNATURES["gp_ball_query_msg_fits"] == [ctypes.c_int] * 3
    fits = _lib.lib().gp_ball_query_msg_fits
    for ns0, ns1 in [(16, 32), (32, 64), (8, 16), (5, 70)]:
        edge = (60 * 1024 - 16 * (ns0 + ns1 + 2)) // 12
        assert fits(edge, ns0, ns1) == 1 and fits(edge + 1, ns0, ns1) == 0, (ns0, ns1, edge)
    assert fits(5053, 16, 32) == 1 and fits(5054, 16, 32) == 0
    assert fits(1, 1, 1) == 1 and fits(0, 16, 32) == 0 and fits(1024, 0, 32) == 0 and fits(1024, 16, -1) == 0
    assert fits(2**31 - 1, 16, 32) == 0  # sized in size_t: no wrap-around into "fits"
    one = ctypes.c_void_p(16)  # (never dereferenced: the entry returns before any launch)
    assert _lib.lib().gp_ball_query_msg_arith(1, 1, 5054, 2, 0.1, 16, 0.2, 32, one, one, one, one, None) == -1
    assert _lib.lib().gp_ball_query_msg(1, 5054, 2, 0.1, 16, 0.2, 32, one, one, one, one, None) == -1


def test_pointnet2_cuda_surface_matches_reference_names():
    """The nine pybind names of pointnet2_api.cpp:10-24."""
    import genpose_amd.pointnet2_cuda as m
    names = ["ball_query_wrapper", "group_points_wrapper", "group_points_grad_wrapper", "gather_points_wrapper",
             "gather_points_grad_wrapper", "furthest_point_sampling_wrapper", "three_nn_wrapper", "three_interpolate_wrapper",
             "three_interpolate_grad_wrapper"]
    for n in names:
        assert callable(getattr(m, n))
    x = torch.zeros(1, 8, 3)
    with pytest.raises(RuntimeError):  # CPU tensors are rejected like CHECK_CUDA (ball_query.cpp:12)
        m.ball_query_wrapper(1, 8, 8, 0.1, 4, x, x, torch.zeros(1, 8, 4, dtype=torch.int32))


def test_no_cpu_fallback():
    from genpose_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.GenposeHipError):
        _lib.check_device()
    from genpose_amd.encoder import Pointnet2EncoderHIP
    enc = Pointnet2EncoderHIP(go.make_state_dict(0, "score"), "cpu")
    with pytest.raises(_lib.GenposeHipError):
        enc.forward(torch.zeros(1, 1024, 3))


def test_pack_weight_layout():
    from genpose_amd.weights import pack_weight
    W = torch.arange(20 * 37, dtype=torch.float32).reshape(20, 37)
    p = pack_weight(W)
    NC, KG = 2, 3
    assert p.numel() == NC * KG * 256
    p = p.reshape(KG, NC, 64, 4)
    for kg in range(KG):
        for nc in range(NC):
            for lane in (0, 5, 17, 63):
                for jj in range(4):
                    n, k = nc * 16 + (lane & 15), kg * 16 + 4 * (lane >> 4) + jj
                    exp = W[n, k].item() if (n < 20 and k < 37) else 0.0
                    assert p[kg, nc, lane, jj].item() == exp


def test_bn_folding_equals_conv_bn():
    """weights.SAScale folds eval-BatchNorm into the 1x1 conv and moves [dx,dy,dz] behind the features."""
    sd = go.make_state_dict(0, "score")
    prefix = "pts_encoder.SA_modules.1.mlps.0."
    x = torch.randn(2, 99, 5, 7)
    ref = go._shared_mlp(sd, prefix, x)
    cur = torch.cat([x[:, 3:], x[:, :3]], dim=1)  # kernel input order: features first, then dx,dy,dz
    for l in range(3):
        p = f"{prefix}layer{l}."
        W = sd[p + "conv.weight"].double().reshape(sd[p + "conv.weight"].shape[0], -1)
        scale = sd[p + "bn.bn.weight"].double() / torch.sqrt(sd[p + "bn.bn.running_var"].double() + 1e-5)
        Wf = W * scale[:, None]
        bf = sd[p + "bn.bn.bias"].double() - sd[p + "bn.bn.running_mean"].double() * scale
        if l == 0:
            Wf = torch.cat([Wf[:, 3:], Wf[:, :3]], dim=1)
        cur = torch.relu(torch.einsum("oc,bchw->bohw", Wf.float(), cur) + bf.float()[None, :, None, None])
    np.testing.assert_allclose(cur.numpy(), ref.numpy(), rtol=1e-4, atol=1e-5)
    from genpose_amd.weights import EncoderWeights
    ew = EncoderWeights(sd, "cpu")
    assert ew.out_dim == 1024 and [s.couts for s in ew.levels[2]] == [[128, 196, 256], [128, 196, 256]]


def test_spread_layout_of_a_partly_filled_hidden_block_is_the_same_network():
    """GP_SA_TAIL_SPREAD (genpose_hip.h): the channels of the last, partly filled 16-channel block of a hidden layer move to positions
    4 (c % 4) + c / 4 of that block, as rows of layer 2 and columns of layer 3 alike.  Host side only: the position map, and that the
    packed streams of the light encoder's 196-wide level multiply out to the plain layers (unpacked with the documented A-fragment
    layout, gp_common.h) - so any kernel that multiplies every position computes the same function."""
    from genpose_amd import _lib
    from genpose_amd.weights import EncoderWeights
    pos = [_lib.lib().gp_sa_tail_position(196, c) for c in range(196)]
    assert pos[:192] == list(range(192)) and pos[192:] == [192, 196, 200, 204]
    assert [_lib.lib().gp_sa_tail_position(40, c) for c in range(32, 40)] == [32, 36, 40, 44, 33, 37, 41, 45]
    assert [_lib.lib().gp_sa_tail_position(64, c) for c in (0, 47, 63)] == [0, 47, 63]  # full blocks keep their order
    assert _lib.lib().gp_sa_tail_position(196, 196) < 0 and _lib.lib().gp_sa_tail_position(0, 0) < 0
    sd = go.make_state_dict(0, "score")
    sc = EncoderWeights(sd, "cpu").levels[2][1]
    assert sc.hidden_layout == 1 and EncoderWeights(sd, "cpu").levels[1][0].hidden_layout == 0

    def unpack(p, n_pad, k_pad):  # [kg][nc][lane][jj] -> W[n][k]
        p = p.reshape(k_pad // 16, n_pad // 16, 64, 4)
        W = torch.zeros(n_pad, k_pad)
        for lane in range(64):
            for jj in range(4):
                W[(lane & 15)::16, (4 * (lane >> 4) + jj)::16] = p[:, :, lane, jj].T
        return W

    prefix = "pts_encoder.SA_modules.2.mlps.1."
    fold = []
    for l in range(3):
        q = f"{prefix}layer{l}."
        W = sd[q + "conv.weight"].double().reshape(sd[q + "conv.weight"].shape[0], -1)
        scale = sd[q + "bn.bn.weight"].double() / torch.sqrt(sd[q + "bn.bn.running_var"].double() + 1e-5)
        fold.append(((W * scale[:, None]).float(), (sd[q + "bn.bn.bias"].double() - sd[q + "bn.bn.running_mean"].double() * scale).float()))
    (w2p, b2p), (w3p, _) = sc.layers[1], sc.layers[2]
    W2s, W3s = unpack(w2p, 208, 128), unpack(w3p, 256, 208)
    h1 = torch.randn(37, 128).abs()
    plain = torch.relu(h1 @ fold[1][0].T + fold[1][1]) @ fold[2][0].T
    spread = torch.relu(h1 @ W2s.T + b2p) @ W3s.T
    np.testing.assert_allclose(spread.numpy(), plain.numpy(), rtol=1e-5, atol=1e-5)
    live = torch.zeros(208, dtype=torch.bool)
    live[pos] = True
    assert W2s[~live].abs().max() == 0 and W3s[:, ~live].abs().max() == 0 and b2p[~live].abs().max() == 0


def test_launch_plans_are_consistent():
    """Host side of the launch plans: the RK45 stage kernels take the sampler's plan (16 / 32-row tiles, 128-row chain form for large
    score-model launches); the forward + backward models stay on 16-row tiles; groups whose rows do not split are refused."""
    import ctypes
    from genpose_amd import _lib
    L = _lib.lib()
    assert L.gp_rk45_plan_rows(0, 1, 64, 50) == 16 and L.gp_rk45_plan_rows(0, 10, 64, 50) == 128
    # forward + backward right-hand sides (energy model's score, likelihood): 16-row tiles, or the 128-row chain form for large launches
    assert L.gp_rk45_plan_rows(1, 1, 64, 50) == 16 and L.gp_rk45_plan_rows(2, 1, 64, 50) == 16
    assert L.gp_rk45_plan_rows(1, 10, 64, 50) == 128 and L.gp_rk45_plan_rows(2, 10, 64, 50) == 128
    assert L.gp_rk45_plan_rows(1, 10, 64, 10) == 16  # k < 43: no chain form
    assert L.gp_pc_layout(1, 0, 10, 64, 50, ctypes.byref(ctypes.c_int(0)), ctypes.byref(ctypes.c_int(0))) == 0
    assert L.gp_pc_layout(1, 32, 1, 64, 50, ctypes.byref(ctypes.c_int(0)), ctypes.byref(ctypes.c_int(0))) != 0  # no 32-row form of the backward pass
    assert L.gp_rk45_plan_rows(0, 10, 64, 10) in (16, 32)  # k < 43: a 128-row workgroup would span more clouds than it stages
    assert L.gp_rk45_plan_rows(0, 0, 64, 50) < 0 and L.gp_rk45_plan_rows(3, 1, 64, 50) < 0
    t, n = ctypes.c_int(0), ctypes.c_int(0)
    assert L.gp_pc_layout(0, 0, 10, 64, 50, ctypes.byref(t), ctypes.byref(n)) == 0 and t.value == L.gp_rk45_plan_rows(0, 10, 64, 50)
    assert L.gp_pc_layout(0, 128, 2, 3, 50, ctypes.byref(t), ctypes.byref(n)) != 0  # 150 rows per batch: a workgroup would straddle two


def test_scorenet_weight_block_shapes():
    from genpose_amd.weights import ScoreNetWeights
    w = ScoreNetWeights(go.make_state_dict(0, "energy"), "cpu")
    t = w.tensors
    assert t["w_headp"].numel() == 48 * 64 * 256 and t["w_headx"].numel() == 48 * 16 * 256
    assert t["w_t1"].shape == (128, 128) and t["w_headt"].shape == (128, 768) and t["w_out"].shape == (9, 256)
    bad = {k: v for k, v in go.make_state_dict(0, "score").items() if "fusion_tail_trans" not in k}
    with pytest.raises(KeyError):
        ScoreNetWeights(bad, "cpu")


def test_pc_schedule_matches_reference_expressions():
    from genpose_amd.samplers import pc_schedule
    ts, sched = pc_schedule(100)
    ref_ts = torch.linspace(1.0, 1e-5, 100)
    assert torch.equal(ts, ref_ts)
    bt = torch.ones(7, 1) * ref_ts[13]
    assert torch.allclose(sched[13, 0], go.ve_sigma(bt)[0, 0], rtol=1e-6)
    assert torch.allclose(sched[13, 1], go.ve_diffusion(bt)[0, 0], rtol=1e-6)
    assert sched[13, 2] == ref_ts[0] - ref_ts[1] and sched[13, 3] == torch.sqrt(ref_ts[0] - ref_ts[1])


def test_rotation_helpers_match_oracle():
    from genpose_amd import rotation
    g = torch.Generator().manual_seed(2)
    r6 = torch.randn(50, 6, generator=g, dtype=torch.float64)
    R = rotation.get_rot_matrix(r6)
    np.testing.assert_allclose(R.numpy(), go.get_rot_matrix(r6).numpy(), atol=1e-14)
    np.testing.assert_allclose(rotation.normalize_rotation(r6).numpy(), go.normalize_rotation(r6).numpy(), atol=1e-14)
    q = rotation.matrix_to_quaternion(R)
    np.testing.assert_allclose(q.numpy(), orot.matrix_to_quaternion(R).numpy(), atol=1e-14)
    np.testing.assert_allclose(rotation.quaternion_to_matrix(q).numpy(), R.numpy(), atol=1e-12)
    Q = q.reshape(5, 10, 4).float()
    a, b = rotation.average_quaternion_batch(Q), go.average_quaternion_batch(Q)
    np.testing.assert_allclose(a.numpy(), b.numpy(), atol=1e-5)
    pose = torch.cat([r6, torch.randn(50, 3, generator=g, dtype=torch.float64)], dim=1)
    np.testing.assert_allclose(rotation.pose9_to_RT(pose).numpy(), go.pose9_to_RT(pose), atol=1e-14)


def test_add_noise_to_RT_golden(golden):
    """runner.add_noise_to_RT against the reference's own output (logged draws + resulting init_x in G9 frame 0)."""
    from genpose_amd.runner import add_noise_to_RT
    g = golden("g9_track.npz")
    draws = [torch.from_numpy(g[f"f0_noise_draw{d}"]) for d in range(4)]
    RT = add_noise_to_RT(torch.from_numpy(g["gt_RT"]), draws=draws)
    cen = torch.from_numpy(g["frames"][0]).mean(dim=1)
    init_x = torch.cat([RT[:, :3, 0], RT[:, :3, 1], RT[:, :3, 3] - cen], dim=-1)
    np.testing.assert_allclose(init_x.numpy(), g["f0_init_x"], atol=1e-6)


def test_config_and_agent_errors():
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    cfg = get_config(device="cpu", sampler_mode=["pc"], sampling_steps=5)
    agent = PoseNet(cfg)
    with pytest.raises(ValueError):  # posenet_agent.py:160
        agent.load_ckpt(model_dir="/nonexistent/ckpt_genpose.pth", model_path=True, load_model_only=True)
    with pytest.raises(NotImplementedError):  # posenet.py:178-179
        agent.net({"pts": torch.zeros(1, 8, 3)}, mode="bogus")
    with pytest.raises(RuntimeError):
        agent.net({"pts": torch.zeros(1, 1024, 3)}, mode="pts_feature")  # no weights loaded
    with pytest.raises(ValueError):
        get_config(nonexistent_flag=1)
    with pytest.raises(NotImplementedError):
        PoseNet(get_config(device="cpu", sde_mode="vp"))
    with pytest.raises(NotImplementedError):
        PoseNet(get_config(device="cpu", pts_encoder="pointnet"))


def test_load_ckpt_accepts_reference_checkpoint_layout(tmp_path):
    """A torch.save'd dict with 'model_state_dict' under the reference key schema loads (weights packed on the CPU)."""
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    path = tmp_path / "ckpt_genpose.pth"
    torch.save({"clock": {}, "model_state_dict": go.make_state_dict(3, "score"), "optimizer_state_dict": {}, "scheduler_state_dict": {}}, path)
    agent = PoseNet(get_config(device="cpu"))
    agent.load_ckpt(model_dir=str(path), model_path=True, load_model_only=True)
    assert agent.net.pts_encoder.out_dim == 1024


def test_synth_is_deterministic_and_real275_shaped():
    from genpose_amd import synth
    a, b = synth.make_batch(6, start=3), synth.make_batch(6, start=3)
    assert a.shape == (6, 1024, 3) and a.dtype == np.float32 and np.array_equal(a, b)
    assert 0.3 < a[..., 2].min() and a[..., 2].max() < 1.6  # metres in front of the camera
    assert np.allclose(a[..., 2] * 1000, np.round(a[..., 2] * 1000), atol=1e-3)  # 1 mm depth quantisation
    g = synth.golden_clouds()
    assert len(np.unique(g[2], axis=0)) < 1024  # tiled duplicates present (FPS ties)


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under genpose_amd/ may import it, and bench.py / __graft_entry__.py only
    inside the CPU-baseline leg and smoke() (as the checker).  Checked on the import statements of every product module and by
    importing the whole package with `oracle` made unimportable."""
    import ast
    import importlib
    import pathlib
    import sys
    root = pathlib.Path(__file__).resolve().parents[1]
    for path in sorted((root / "genpose_amd").glob("*.py")):
        tree = ast.parse(path.read_text())
        for node in ast.walk(tree):
            names = []
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                names = [node.module or ""]
            assert not any(n == "oracle" or n.startswith("oracle.") for n in names), f"{path.name} imports the oracle"
    # bench.py: the only oracle import sits inside run_cpu_baseline; __graft_entry__.py: inside smoke()/build()
    for fname, allowed in (("bench.py", {"run_cpu_baseline"}), ("__graft_entry__.py", {"smoke", "build"})):
        tree = ast.parse((root / fname).read_text())
        for fn in [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)]:
            for node in ast.walk(fn):
                mods = [a.name for a in node.names] if isinstance(node, ast.Import) else ([node.module or ""] if isinstance(node, ast.ImportFrom) else [])
                if any(m == "oracle" or m.startswith("oracle.") for m in mods):
                    assert fn.name in allowed, f"{fname}:{fn.name} imports the oracle"
        for node in tree.body:  # module level
            mods = [a.name for a in node.names] if isinstance(node, ast.Import) else ([node.module or ""] if isinstance(node, ast.ImportFrom) else [])
            assert not any(m == "oracle" or m.startswith("oracle.") for m in mods), f"{fname} imports the oracle at module level"

    class _Block:
        def find_spec(self, name, path=None, target=None):
            if name == "oracle" or name.startswith("oracle."):
                raise ImportError("the oracle is not available to the product")
            return None

    saved = {k: v for k, v in sys.modules.items() if k == "oracle" or k.startswith("oracle.") or k == "genpose_amd" or k.startswith("genpose_amd.")}
    for k in saved:
        del sys.modules[k]
    sys.meta_path.insert(0, _Block())
    try:
        for path in sorted((root / "genpose_amd").glob("*.py")):
            if path.stem not in ("__init__", "build"):
                importlib.import_module(f"genpose_amd.{path.stem}")
    finally:
        sys.meta_path.pop(0)
        for k in [k for k in sys.modules if k == "genpose_amd" or k.startswith("genpose_amd.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_bench_spawns_the_documented_launch_line(monkeypatch):
    """`python bench.py --gpus N` with no launcher environment re-executes itself under torch.distributed.run, one rank per GPU,
    rendezvous on 127.0.0.1 (the container hostname may not resolve)."""
    import argparse
    import subprocess
    import sys as _sys
    import bench
    seen = {}

    class FakeProc:
        def __init__(self, cmd, env=None, stdout=None, text=None):
            seen["cmd"], seen["env"] = cmd, env
            self.stdout = iter(seen.get("lines", ['{"metric": "x", "value": 1.0}\n']))

        def wait(self):
            return seen.get("rc", 0)

    monkeypatch.setattr(subprocess, "Popen", FakeProc)
    monkeypatch.setattr(_sys, "argv", ["bench.py", "--gpus", "8", "--steps", "20", "--warmup", "5"])
    assert bench.self_launch(argparse.Namespace(gpus=8, steps=20, warmup=5)) == 0
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=8" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    assert cmd[-6:] == ["--gpus", "8", "--steps", "20", "--warmup", "5"] and cmd[-7].endswith("bench.py")
    assert seen["env"]["GP_BENCH_LAUNCH"] == "self" and seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_bench_prints_a_line_when_the_launcher_dies_without_one(monkeypatch, capsys):
    """A launcher that ends without rank 0's JSON line (a crash before Python starts, an OOM kill) still yields ONE parseable line with an
    "error" field - the driver's multi-GPU run must come back diagnosable, not empty."""
    import argparse
    import json
    import subprocess
    import sys as _sys
    import bench

    class FakeProc:
        def __init__(self, cmd, env=None, stdout=None, text=None):
            self.stdout = iter(["some launcher chatter\n"])

        def wait(self):
            return 9

    monkeypatch.setattr(subprocess, "Popen", FakeProc)
    monkeypatch.setattr(_sys, "argv", ["bench.py", "--gpus", "4"])
    assert bench.self_launch(argparse.Namespace(gpus=4, steps=20, warmup=3)) == 9
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["value"] is None and line["n_gpus"] == 4 and "exited with code 9" in line["error"]


def test_shape_cache_evicts_least_recently_used_and_skips_pins():
    """lru.ShapeCache: the bounded per-shape caches of the host side (samplers, staging buffers, encoder workspaces, captured passes)."""
    from genpose_amd.lru import ShapeCache
    ev = []
    c = ShapeCache(3, can_evict=lambda v: not v.get("pin"), on_evict=lambda k, v: ev.append(k))
    c["a"] = {"pin": True}
    c["b"] = {}
    c["c"] = {}
    assert c.get("b") is not None  # b is now the most recently used
    c["d"] = {}
    assert list(c.keys()) == ["a", "b", "d"] and ev == ["c"]  # a is pinned; c was the least recently used unpinned entry
    c["e"] = {}
    assert list(c.keys()) == ["a", "d", "e"] and ev == ["c", "b"]
    assert "a" in c and c["a"]["pin"] and len(c) == 3 and c.get("zzz") is None
    with pytest.raises(KeyError):
        c["zzz"]
    c["f"] = {"pin": True}
    c["g"] = {"pin": True}
    assert all(v.get("pin") for v in c.values())  # nothing evictable is left: the cache exceeds its soft capacity rather than drop a pin
    # every way OUT of the cache runs on_evict (an entry that pinned workspaces gives them back): pop, overwrite, clear
    ev2 = []
    d = ShapeCache(4, on_evict=lambda k, v: ev2.append((k, v["id"])))
    d["x"], d["y"], d["z"] = {"id": 1}, {"id": 2}, {"id": 3}
    assert d.pop("x")["id"] == 1 and d.pop("nope", "dflt") == "dflt" and ev2 == [("x", 1)]
    d["y"] = {"id": 22}                                      # overwrite: the old entry is dropped
    same = d["z"]
    d["z"] = same                                            # re-inserting the same object is not a drop
    assert ev2 == [("x", 1), ("y", 2)]
    d.clear()
    assert sorted(ev2[2:]) == [("y", 22), ("z", 3)] and len(d) == 0
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    net = PoseNet(get_config(device="cpu")).net
    assert isinstance(net._samplers, ShapeCache) and net._samplers.capacity == net.MAX_SAMPLERS == 8


def test_bench_dump_outputs_types_and_size_cap(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float32 stays float32, float64 and integers become float64, None is left out; above the size limit every
    array keeps a fixed, seeded, ordered sample of its leading-axis entries (the same sample in every run)."""
    import bench
    pose = torch.arange(40 * 3, dtype=torch.float32).reshape(40, 3)
    arrays = {"pose": pose, "pose64": pose.double(), "order": torch.arange(40), "none": None}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    got = {f.stem: np.load(f) for f in (tmp_path / "a").iterdir()}
    assert set(got) == {"pose", "pose64", "order"}
    assert got["pose"].dtype == np.float32 and got["pose64"].dtype == np.float64 and got["order"].dtype == np.float64
    assert np.array_equal(got["pose"], pose.numpy()) and np.array_equal(got["order"], np.arange(40))
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1024)
    for run in ("b", "c"):
        bench.dump_outputs(str(tmp_path / run), arrays)
    b = {f.stem: np.load(f) for f in (tmp_path / "b").iterdir()}
    c = {f.stem: np.load(f) for f in (tmp_path / "c").iterdir()}
    assert sum(a.nbytes for a in b.values()) <= 1024
    rows = b["order"].astype(np.int64)
    assert len(rows) < 40 and np.all(np.diff(rows) > 0) and np.array_equal(b["pose"], pose.numpy()[rows])
    assert all(np.array_equal(b[k], c[k]) for k in b)
