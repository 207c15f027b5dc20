"""Vanilla PointNet encoder on the HIP kernels - drop-in for `PointNetfeat(num_points, out_dim=1024)` fed `pts.permute(0, 2, 1)`
(networks/pts_encoder/pointnets.py:83-123; the agent's cfg.pts_encoder = 'pointnet' | 'pointnet_and_pointnet2', networks/posenet.py:36-46).

forward(pts [B,n,3] f32 on the GPU) -> [B,1024], any n >= 1.  Launch sequence per call (one stream, in this order, csrc/pointnet.hip):
  gp_pointnet_stn_pool   transform net's convolutions 3-64-128-1024 + max over the cloud   -> g [B,1024]
  3 x gp_dense_rows      its head fc1 - fc2 - fc3 (+ identity, folded into fc3's bias)      -> trans [B,3,3]
  gp_pointnet_feat_pool  x . trans, trunk 3-64-128-512-1024 (conv4 without ReLU) + max     -> feat [B,1024]
The reference's [B,1024,n] and [B,512,n] activations never exist: a workspace holds per-cloud vectors only (11 KiB per cloud).
"""
import torch

from . import _lib
from ._lib import ptr, stream_ptr
from .graphs import CapturedPasses, capture, pin, unpinned
from .lru import ShapeCache
from .weights import PointNetWeights

ACT_NONE, ACT_RELU = 0, 1  # GP_ACT_* (include/genpose_hip.h)


def dense_rows(xa, W, bias, act=ACT_NONE, xb=None, out=None):
    """out [rows, n_out] = act([xa | xb] . W^T + bias) on the device (gp_dense_rows); W [n_out, k_a + k_b] as trained."""
    rows, ka = xa.shape
    kb = 0 if xb is None else xb.shape[1]
    n_out = W.shape[0]
    if W.shape[1] != ka + kb or (xb is not None and xb.shape[0] != rows):
        raise ValueError(f"dense_rows: inputs [{rows}, {ka} + {kb}] against a weight {tuple(W.shape)}")
    if out is None:
        out = torch.empty(rows, n_out, device=xa.device, dtype=torch.float32)
    _lib.call("gp_dense_rows", rows, ka, kb, n_out, ptr(xa), ptr(xb), ptr(W), ptr(bias), act, ptr(out), stream_ptr())
    return out


class PointNetEncoderHIP:
    MAX_WORKSPACES = 12
    MAX_PASS_GRAPHS = 8  # captured passes kept (least recently used first)

    def __init__(self, state_dict, device="cuda", prefix="pts_encoder."):
        self.device = torch.device(device)
        self.w = PointNetWeights(state_dict, self.device, prefix)
        self.out_dim = self.w.out_dim
        self._ws = ShapeCache(self.MAX_WORKSPACES, can_evict=unpinned)
        self._pass_graphs = CapturedPasses(self.MAX_PASS_GRAPHS)

    # ------------------------------------------------------------------ workspace (cached per batch / size)
    def _workspace(self, B, n):
        ws = self._ws.get((B, n))
        if ws is None:
            dev = self.device
            ws = self._ws[(B, n)] = {"g": torch.empty(B, 1024, device=dev), "h1": torch.empty(B, 512, device=dev), "h2": torch.empty(B, 256, device=dev),
                                     "trans": torch.empty(B, 3, 3, device=dev), "feat": torch.empty(B, 1024, device=dev)}
        return ws

    def workspace_bytes(self, B, n):
        """Device bytes this encoder holds for the geometry (B, n): the per-cloud vectors, plus the static input of a captured pass."""
        total = sum(t.numel() * t.element_size() for t in self._workspace(B, n).values() if torch.is_tensor(t))
        ent = self._pass_graphs.get((B, n, 3))
        if ent is not None:  # static input [B,n,3] and static output [B,1024] of the captured pass
            total += sum(t.numel() * t.element_size() for t in (*ent.bufs, ent.outs))
        return total

    # ------------------------------------------------------------------ the pass
    def forward(self, pts, return_trans=False):
        _lib.check_device()
        if not pts.is_cuda or pts.dtype != torch.float32:
            raise RuntimeError("pts must be a float32 CUDA tensor")
        xyz = pts[..., 0:3].contiguous()
        B, n, _ = xyz.shape
        if n < 1:
            raise _lib.GenposeHipError("PointNetEncoderHIP needs at least one point per cloud")
        ws = self._workspace(B, n)
        st = stream_ptr()
        (w1, b1), (w2, b2), (w3, b3) = self.w.stn_convs
        _lib.call("gp_pointnet_stn_pool", B, n, ptr(xyz), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(w3), ptr(b3), ptr(ws["g"]), st)
        (f1, c1), (f2, c2), (f3, c3) = self.w.stn_fcs
        dense_rows(ws["g"], f1, c1, ACT_RELU, out=ws["h1"])
        dense_rows(ws["h1"], f2, c2, ACT_RELU, out=ws["h2"])
        dense_rows(ws["h2"], f3, c3, ACT_NONE, out=ws["trans"].view(B, 9))
        (w1, b1), (w2, b2), (w3, b3), (w4, b4) = self.w.convs
        _lib.call("gp_pointnet_feat_pool", B, n, ptr(xyz), ptr(ws["trans"]), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(w3), ptr(b3), ptr(w4), ptr(b4),
                  ptr(ws["feat"]), st)
        feat = ws["feat"].clone()
        return (feat, ws["trans"].clone()) if return_trans else feat

    __call__ = forward

    def encode(self, pts, use_graph=True):
        """The pass as one hipGraph replay per input shape (as Pointnet2EncoderHIP.encode): the first call of a shape runs launch by
        launch, the second captures - one stream, launch order, no parallel branches -, later ones copy the clouds into the graph's static
        input and replay.  Results are the launch-by-launch pass's, bit for bit (same kernels; the cross-tile maximum is order-independent)."""
        if not use_graph or not pts.is_cuda or pts.dtype != torch.float32 or torch.cuda.is_current_stream_capturing():
            return self.forward(pts)
        key = (pts.shape[0], pts.shape[1], 3)

        def captured():
            buf = pts[..., 0:3].contiguous().clone()
            # (no warm-up: the first call of the shape was one; the workspace is allocated and pinned BEFORE the capture: the replay writes into it)
            return capture(lambda: self.forward(buf), bufs=(buf,), pins=[lambda: pin(self._workspace(key[0], key[1]))])
        ent = self._pass_graphs.entry(key, key, captured)
        if ent is None:
            return self.forward(pts)
        return ent.replay(pts[..., 0:3]).clone()
