"""GPU: the caches of captured graphs (genpose_amd/graphs.py) keep their pins balanced across eviction and recapture, in the frame graphs'
two-network and one-network forms and in both encoders' encode().  1024-point clouds, 1 .. MAX_SHAPES + 1 of them; no ODE solve."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from genpose_amd import synth
from genpose_amd.weights_synth import make_state_dict


@functools.lru_cache(maxsize=None)
def _state_dict(mode, pts_encoder="pointnet2"):
    return make_state_dict(0, mode, pts_encoder=pts_encoder)


@functools.lru_cache(maxsize=None)
def _clouds(n):
    return torch.from_numpy(synth.make_batch(n, start=300 + 10 * n)).cuda().float()


def _net(mode):
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    agent = PoseNet(get_config(posenet_mode=mode, sampler_mode=["ode"]))
    agent.load_state_dict(_state_dict(mode))
    agent.net._need_weights()
    return agent.net


def _pins(net):
    return sum(ws.get("_pins", 0) for ws in net.pts_encoder._ws.values())


def _snapshot(fg, outs):
    if fg.ev_e is not None:
        torch.cuda.current_stream().wait_event(fg.ev_e)  # the energy model's embedding comes from the side stream
    return [None if t is None else t.clone() for t in outs]


def _evict_and_recapture(nets):
    from genpose_amd.runner import _FrameGraphs
    fg = _FrameGraphs(*nets, K=6, sel=3)
    M = fg.MAX_SHAPES
    first = None
    for n in range(1, M + 2):  # one shape more than the cache holds: capturing the last evicts n = 1
        for _ in range(2):
            outs = fg.embed(_clouds(n))
        if n == 1:
            first = _snapshot(fg, outs)
            assert len(fg._a) == 1 and all(_pins(net) == 1 for net in nets)
    assert len(fg._a) == M and (tuple(_clouds(1).shape), torch.float32) not in fg._a
    for net in nets:  # one pin per live entry: the evicted entry gave its pin back
        assert _pins(net) == M
    again = _snapshot(fg, fg.embed(_clouds(1)))  # a recapture, which evicts n = 2
    assert len(fg._a) == M and all(_pins(net) == M for net in nets)
    eager = [_clouds(1).mean(dim=1)] + [net.pose_score_net.cloud_embed(net.pts_encoder.forward(_clouds(1), slot=0)) for net in nets]
    for got, before, want in zip(again, first, eager):
        assert torch.equal(got, before) and torch.equal(got, want)
    fg._a.clear()
    assert all(_pins(net) == 0 for net in nets)
    return fg, again


def test_two_networks_pins_follow_eviction_and_a_recapture_has_the_same_bits():
    fg, (centre, cvec_s, cvec_e) = _evict_and_recapture((_net("score"), _net("energy")))
    assert fg.SLOT == "frame-graphs" and fg.ev_e is not None and cvec_e.shape == cvec_s.shape == (1, 768)


def test_one_network_is_graph_a_alone():
    fg, (centre, cvec_s, cvec_e) = _evict_and_recapture((_net("score"),))
    assert fg.SLOT == "fixed-step-tracker" and cvec_e is None
    assert fg.ev_e is None and fg.side is None  # no side stream work is recorded


@pytest.mark.parametrize("which", ["pointnet2", "pointnet"])
def test_encode_runs_direct_then_captures_then_replays(which):
    if which == "pointnet2":
        from genpose_amd.encoder import Pointnet2EncoderHIP
        enc = Pointnet2EncoderHIP(_state_dict("score"), "cuda")
        encode = lambda: enc.encode(_clouds(2))[0]
    else:
        from genpose_amd.pointnet_encoder import PointNetEncoderHIP
        enc = PointNetEncoderHIP(_state_dict("score", "pointnet"), "cuda")
        encode = lambda: enc.encode(_clouds(2))
    direct = encode()
    assert len(enc._pass_graphs) == 0 and [ws.get("_pins", 0) for ws in enc._ws.values()] == [0]
    captured = encode()
    assert len(enc._pass_graphs) == 1
    replayed = encode()
    assert len(enc._pass_graphs) == 1 and all(ent.graph is not None for ent in enc._pass_graphs.values())
    assert torch.equal(direct, captured) and torch.equal(direct, replayed) and bool(torch.isfinite(direct).all())
    assert [ws["_pins"] for ws in enc._ws.values()] == [1]
    enc._pass_graphs.clear()
    assert [ws["_pins"] for ws in enc._ws.values()] == [0]
