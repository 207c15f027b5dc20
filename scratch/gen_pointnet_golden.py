"""Writes tests/golden/g18_pointnet.npz from the REFERENCE's own PointNetfeat and its pointnet_and_pointnet2 agent (CPU, fp32):

    python -m scratch.gen_pointnet_golden          (needs the reference tree: oracle/ref_import.py; nothing on the GPU side does)

  clouds_{B}x{n}, trans_{B}x{n} [B,3,3], feat_{B}x{n} [B,1024]   PointNetfeat(num_points, out_dim=1024) of ns.PoseNet(cfg, pts_encoder='pointnet')
                                                                  at (B, n) = (3, 1024), (2, 37), (1, 1), (2, 1100)
  fused_feat_score / fused_feat_energy [3,1024]                   extract_pts_feature of the pointnet_and_pointnet2 agents on clouds_3x1024
  pc_*                                                            one pred_func of the fused score agent: PC sampler, B = 2, K = 4, 5 steps, the
                                                                  randn / randn_like draws logged as G7's were; pc_energy = get_energy(T=1e-5) of
                                                                  the fused energy agent on its result
Arrays only: the weights are weights_synth.make_state_dict(0, mode, pts_encoder=...), which the tests rebuild from the seed.
"""
import argparse
import os

import numpy as np
import torch

from genpose_amd import synth
from genpose_amd.weights_synth import make_state_dict
from oracle import ref_import
from oracle.gen_golden import OUT, DrawLog

SHAPES = ((3, 1024), (2, 37), (1, 1), (2, 1100))


def clouds(B, n):
    """[B,n,3] float32: synthetic clouds cut to n points; beyond 1024 the head of the next cloud is appended."""
    a = synth.make_batch(B + 1, start=300 + n)
    return np.ascontiguousarray(np.concatenate([a[:B], a[1:B + 1]], axis=1)[:, :n]).astype(np.float32)


def agent_of(ns, mode, pts_encoder, sampler="pc", steps=5):
    cfg = argparse.Namespace(**vars(ns.cfg))
    cfg.posenet_mode, cfg.sampler_mode, cfg.sampling_steps, cfg.pts_encoder = mode, [sampler], steps, pts_encoder
    agent = ns.PoseNet(cfg)
    agent.net.load_state_dict(make_state_dict(0, mode, pts_encoder=pts_encoder), strict=True)
    agent.net.eval()
    return agent


def main():
    torch.set_num_threads(8)
    ns = ref_import.load(sampler_mode="pc")
    out = {}
    with torch.no_grad():
        enc = agent_of(ns, "score", "pointnet").net.pts_encoder  # PointNetfeat
        for B, n in SHAPES:
            c = clouds(B, n)
            x = torch.from_numpy(c).permute(0, 2, 1)
            trans, feat = enc.stn(x).numpy(), enc(x).numpy()
            assert (feat < 0).any(), "the pooled trunk output must have negative entries (signed maximum)"
            assert np.abs(trans - np.eye(3, dtype=np.float32)).max() > 0.1, "trans must differ visibly from the identity"
            out[f"clouds_{B}x{n}"], out[f"trans_{B}x{n}"], out[f"feat_{B}x{n}"] = c, trans, feat
        sa, ea = agent_of(ns, "score", "pointnet_and_pointnet2"), agent_of(ns, "energy", "pointnet_and_pointnet2")
        pts = torch.from_numpy(out["clouds_3x1024"])
        out["fused_feat_score"] = sa.net.extract_pts_feature({"pts": pts.clone()}).numpy()
        out["fused_feat_energy"] = ea.net.extract_pts_feature({"pts": pts.clone()}).numpy()
    pts2 = pts[:2].clone()
    cen2 = pts2.mean(dim=1)
    torch.manual_seed(218)
    with DrawLog() as dl:
        pred, proc = sa.pred_func({"pts": pts2.clone(), "pts_center": cen2.clone()}, repeat_num=4, save_path=None, return_process=True)
    assert len(dl.draws) == 11  # the prior, then (Langevin, predictor) per step
    energy = ea.get_energy(data={"pts": pts2.clone(), "pts_center": cen2.clone()}, pose_samples=pred, T=1e-5)
    out.update(pc_prior_noise=dl.draws[0].numpy(), pc_z_langevin=torch.stack(dl.draws[1::2]).numpy(), pc_z_predictor=torch.stack(dl.draws[2::2]).numpy(),
               pc_pred=pred.numpy(), pc_proc=proc.numpy(), pc_energy=energy.detach().numpy())
    path = os.path.join(OUT, "g18_pointnet.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
