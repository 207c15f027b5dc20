"""GPU: the encoder issues exactly the launches its plan lists (Pointnet2EncoderHIP.launch_plan, pinned on the CPU by
tests/test_encoder_plan_host.py), and the launch-by-launch pass, encode() direct and encode() replayed agree bit for bit - with the fp32
kernels, with all three exact-product split-bf16 kernels in use, and with all three asked for below their minimum batches."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import genpose_oracle as go

NB = 2
FRONT_END = {"gp_fps_chain_arith", "gp_furthest_point_sampling_arith", "gp_ball_query_msg_arith", "gp_ball_query_arith"}
SPLIT = dict(precision="bf16x9", level1="bf16x9", level3="bf16x9")
F32, X9, LDS, GA, PL = "gp_sa_pre_mlp_max_layout", "gp_sa_pre_mlp_max_bf16x9", "gp_sa_lds_bf16x9", "gp_sa_groupall_bf16x9", "gp_point_linear"
# (constructor options, both minimum batches or None for the class's, the plan at NB clouds)
SETTINGS = {
    "defaults": ({}, None, [F32, F32, PL, F32, F32, PL, F32, F32, PL, F32, F32]),
    "split": (SPLIT, 1, [F32, F32, PL, LDS, LDS, PL, X9, X9, GA]),
    "split_below_minimum": (SPLIT, 3, [F32, F32, PL, F32, F32, PL, X9, X9, PL, F32, F32]),
}


@functools.lru_cache(maxsize=None)
def _inputs():
    from genpose_amd import synth
    return go.make_state_dict(0, "score"), torch.from_numpy(synth.make_batch(NB, start=11, n_pts=512)).cuda().float()


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_launches_are_the_plan_and_the_three_paths_agree_bit_for_bit(setting, monkeypatch):
    from genpose_amd import _lib
    from genpose_amd.encoder import Pointnet2EncoderHIP
    sd, pts = _inputs()
    kwargs, minimum, plan = SETTINGS[setting]
    enc = Pointnet2EncoderHIP(sd, "cuda", **kwargs)
    if minimum is not None:
        enc.LEVEL1_BF16X9_MIN_CLOUDS = enc.LEVEL3_BF16X9_MIN_CLOUDS = minimum
    assert enc.launch_plan(NB) == plan

    names = []
    real_call = _lib.call

    def recording_call(name, *args):
        names.append(name)
        real_call(name, *args)

    def set_abstraction_launches(run):
        del names[:]
        out = run()
        first = next(i for i, name in enumerate(names) if name not in FRONT_END)
        assert first > 0 and not FRONT_END & set(names[first:])  # the grouping front end comes first, whole
        return out, names[first:]

    monkeypatch.setattr(_lib, "call", recording_call)
    forward, issued = set_abstraction_launches(lambda: enc.forward(pts))
    assert issued == plan
    (direct, _), issued = set_abstraction_launches(lambda: enc.encode(pts))  # first call of a shape: launch by launch
    assert issued == plan
    monkeypatch.undo()
    replayed = [enc.encode(pts)[0] for _ in range(2)]  # capture + replay, then replay
    assert len(enc._pass_graphs) == 1
    torch.cuda.synchronize()
    assert forward.shape == (NB, 1024) and bool(torch.isfinite(forward).all())
    for other in (direct, *replayed):
        assert torch.equal(forward, other)
