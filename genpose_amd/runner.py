"""Runner loops over the agent: the batch / frame loops of runners/evaluation_single.py:309-489 and
runners/evaluation_tracking.py:262-337 restated around the HIP agent.

Inputs  : lists / arrays of [1024,3] float32 clouds (camera frame, metres, NOT centred); for tracking also per-frame
          `model_name`s and an initial sRT per object.
Outputs : multi_hypothesis_pred_RTs [n,K,4,4] (float64, as the reference's numpy RTs), energy [n,K,2], aggregated
          sRT [n,4,4].
Detection pre-processing (depth+mask -> cloud) and mAP evaluation are the "next" rows of SURVEY §8f.
"""
import math

import numpy as np
import torch

from . import _lib, reward, rotation
from .graphs import UploadRing, capture, holding, release
from .lru import ShapeCache


def make_batch_sample(pts):
    """The dict the agents consume (evaluation_single.py:394-403): `pts` stays un-centred, `pts_center` is the mean."""
    pts = pts.float()
    centre = torch.mean(pts[:, :, :3], dim=1)
    return {"pts": pts, "zero_mean_pts": pts - centre.unsqueeze(1), "pts_center": centre}


class _one_cpu_thread:
    """Host-side torch ops inside the per-frame loops run single-threaded: a multi-threaded CPU op leaves its OpenMP team spinning
    next to the HIP runtime's progress thread and the following graph replays stall for tens of milliseconds (EXPERIMENTS.md §G, the tracking history of DESIGN r5 §8)."""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *exc):
        torch.set_num_threads(self.n)


class SingleFrameRunner:
    """inference_pose + inference_energy (evaluation_single.py:356-489) without the pickle round trip in between.

    ranker: 'energy' (default: the energy agent's two energies rank the hypotheses, as the reference) or 'likelihood' (ours: the SCORE
    agent's own exact-divergence log-likelihood, PoseNet.get_likelihood under the agent's cfg.likelihood_solver / likelihood_steps, fills
    both columns of the [n,K,2] array, cast to float32, and goes through the same ranking - no energy agent needed) or 'consensus' (ours: no
    network at all - reward.consensus_rank_aggregate scores every candidate by its mean distance to the cloud's other candidates, rotation
    and translation independently, and ranks and aggregates in the same launch; the stored 'energy' is that array).

    sample_from: 'score' (default) or 'energy' (ours; opt-in) - the ENERGY agent (energy_agent; score_agent may be None) draws the
    candidates itself with its pred_func (a posenet_mode='energy' agent: 'ode' / 'pc', or 'heun' / 'dpm2m' under cfg.fixed_step_energy) and
    then ranks them with get_energy(extract_pts_feature=False) on the cloud features pred_func left in the dict: ONE encoder pass per batch,
    one checkpoint.  ranker 'energy' or 'consensus'; 'likelihood' is refused - likelihoods come from the score model.

    aggregate: 'mean' (default: average_sRT is the quaternion mean and mean translation of the ranker's top max(1, int(K ratio)) candidates,
    as the reference) or 'mode' (ours; opt-in) - the ranking is the same, then reward.mode_aggregate runs on those top candidates per
    column (reward.selection_weight of the ranking's order, made on the device): average_sRT is the mode's 4x4 (mode_RT as float64) and the
    dict gains mode_mass [n,2], the share of the selected candidates the mode explains (rotation, translation).  sym then also tells the
    mode which clouds to compare by their y axis, under every ranker."""

    RANKERS = ("energy", "likelihood", "consensus")
    SAMPLE_FROM = ("score", "energy")
    AGGREGATES = ("mean", "mode")

    def __init__(self, score_agent, energy_agent=None, repeat_num=50, T0=0.55, batch_size=256, ratio=0.6, ranker="energy", sample_from="score",
                 aggregate="mean"):
        if ranker not in self.RANKERS:
            raise NotImplementedError(f"ranker {ranker!r}: one of {self.RANKERS}")
        if aggregate not in self.AGGREGATES:
            raise ValueError(f"SingleFrameRunner(aggregate={aggregate!r}): one of {self.AGGREGATES}")
        if sample_from not in self.SAMPLE_FROM:
            raise ValueError(f"SingleFrameRunner(sample_from={sample_from!r}): one of {self.SAMPLE_FROM}")
        if sample_from == "energy":
            if ranker == "likelihood":
                raise ValueError("SingleFrameRunner(sample_from='energy', ranker='likelihood'): likelihoods come from the score model; "
                                 "ranker 'energy' or 'consensus'")
            if energy_agent is None or energy_agent.cfg.posenet_mode != "energy":
                raise ValueError("SingleFrameRunner(sample_from='energy') needs energy_agent with posenet_mode='energy'"
                                 + ("" if energy_agent is None else f", got {energy_agent.cfg.posenet_mode!r}"))
        self.score_agent, self.energy_agent, self.ranker, self.sample_from = score_agent, energy_agent, ranker, sample_from
        self.repeat_num, self.T0, self.batch_size, self.ratio, self.aggregate = repeat_num, T0, batch_size, ratio, aggregate
        self.depth_front_end = None  # infer_depth's preprocess.DepthToClouds (assign one for other intrinsics / crop size / cloud size)

    def infer_tensors(self, clouds, sym=None):
        """clouds: device tensor [n,1024,3] -> dict of device tensors with leading dim n (usable under ShardedInference).
        sym [n] (ranker 'consensus' or aggregate 'mode' only): clouds of objects symmetric about their y axis, compared by that axis alone."""
        n = clouds.shape[0]
        if sym is not None:
            if self.ranker != "consensus" and self.aggregate != "mode":
                raise ValueError(f"sym is the consensus ranker's argument (ranker={self.ranker!r})")
            sym = torch.as_tensor(sym)
            if sym.shape != (n,):
                raise ValueError(f"sym must hold one flag per cloud ([{n}]), got {tuple(sym.shape)}")
        out = {"pred_pose": [], "multi_hypothesis_pred_RTs": [], "energy": [], "sorted_RTs": [], "average_sRT": [], "mode_mass": []}
        for s in range(0, n, self.batch_size):  # evaluation_single.py:380-382 batch slicing
            sample = make_batch_sample(clouds[s:s + self.batch_size])
            sampling_agent = self.energy_agent if self.sample_from == "energy" else self.score_agent
            pred = sampling_agent.pred_func(data=sample, repeat_num=self.repeat_num, save_path=None, T0=self.T0)
            out["pred_pose"].append(pred)
            out["multi_hypothesis_pred_RTs"].append(rotation.pose9_to_RT(pred))
            r = None
            if self.ranker == "consensus":
                r = reward.consensus_rank_aggregate(pred, None if sym is None else sym[s:s + self.batch_size], ratio=self.ratio)
                out["energy"].append(r["energy"])
                out["sorted_RTs"].append(rotation.pose9_to_RT(r["sorted_poses"]))
                out["average_sRT"].append(rotation.quat_trans_to_RT(r["avg_pose"].double()))
            elif self.ranker == "likelihood" or self.energy_agent is not None:
                if self.ranker == "likelihood":
                    # (pred_func left the clouds' features in the dict) higher = more likely = first, in both columns
                    ll32 = self.score_agent.get_likelihood(sample, pred, extract_pts_feature=False).float()
                    energy = torch.stack([ll32, ll32], dim=-1).contiguous()
                elif self.sample_from == "energy":
                    # (pred_func left the clouds' features - this agent's own - in the dict) no second encoder pass
                    energy = self.energy_agent.get_energy(data=sample, pose_samples=pred, T=1e-5, extract_pts_feature=False)
                else:
                    energy = self.energy_agent.get_energy(data=sample, pose_samples=pred, T=1e-5)  # evaluation_single.py:339-343
                r = reward.rank_aggregate(pred, energy, ratio=self.ratio)
                out["energy"].append(energy)
                out["sorted_RTs"].append(rotation.pose9_to_RT(r["sorted_poses"]))
                out["average_sRT"].append(rotation.quat_trans_to_RT(r["avg_pose"].double()))
            if self.aggregate == "mode" and r is not None:  # the same ranking; the mode of its top candidates replaces their mean
                w = reward.selection_weight(r["order"], max(1, int(pred.shape[1] * self.ratio)))
                m = reward.mode_aggregate(pred, None if sym is None else sym[s:s + self.batch_size], w, with_rt=True)
                out["average_sRT"][-1] = m["mode_RT"].double()
                out["mode_mass"].append(m["mass"])
        return {k: torch.cat(v, dim=0) for k, v in out.items() if v}

    def infer(self, clouds, device="cuda", sym=None):
        """clouds: array-like [n,1024,3].  Returns dict of numpy arrays (+ 'pred_pose' [n,K,9])."""
        clouds = torch.as_tensor(np.asarray(clouds), dtype=torch.float32).to(device)
        return {k: v.cpu().numpy() for k, v in (self.infer_tensors(clouds) if sym is None else self.infer_tensors(clouds, sym)).items()}

    def infer_depth(self, depth, masks, rois, class_ids, seed=0, frame=0):
        """A depth frame and its detections (the inputs of preprocess.DepthToClouds) -> infer_tensors' dict on ALL n detections, plus
        `valid` [n] uint8, `cat_id` [n] (class_ids - 1), `count` and `depth_count` [n]; device tensors throughout.  The clouds come from
        DepthToClouds.device_clouds (self.depth_front_end; a default one on first use): one launch, the sampled pixels a function of
        (seed, frame, detection index), no count read back.  A detection the reference skips (valid = 0: its cloud is all zeros) runs through
        the networks with the rest and gets the identity as average_sRT, the reference's f_sRT[i] = identity - by a device-side select."""
        return self._infer_front_end(lambda fe: fe.device_clouds(depth, masks, rois, seed, frame), np.asarray(class_ids))

    def _infer_front_end(self, clouds, class_ids):
        """clouds(front end) -> its dict; class_ids: host array, one per detection.  infer_tensors on the dict's points, the identity as
        average_sRT where valid = 0, the front end's other fields carried along, cat_id = class_ids - 1."""
        from .preprocess import DepthToClouds
        if self.depth_front_end is None:
            self.depth_front_end = DepthToClouds()
        fe = clouds(self.depth_front_end)
        if len(class_ids) != fe["valid"].shape[0]:
            raise ValueError(f"{len(class_ids)} class_ids for {fe['valid'].shape[0]} detections")
        out = self.infer_tensors(fe["points"])
        if "average_sRT" in out:
            avg = out["average_sRT"]
            out["average_sRT"] = torch.where(fe["valid"].bool().view(-1, 1, 1), avg, torch.eye(4, dtype=avg.dtype, device=avg.device))
        out.update((k, v) for k, v in fe.items() if k != "points")
        out["cat_id"] = torch.as_tensor(class_ids, dtype=torch.int64).to(fe["valid"].device) - 1
        return out

    def infer_depth_frames(self, frames, seed=0, first_frame=0):
        """infer_depth over MANY frames: frames, a sequence of (depth, masks, rois, class_ids) of one image size -> infer_depth's dict over
        all n = sum n_f detections in frame order, plus `frame` and `inst` [n] int64 (which frame, which instance of it).  ONE front-end
        launch (DepthToClouds.device_clouds_frames; frame f draws as (seed, first_frame + f, instance), so its rows are what
        infer_depth(*frames[f], seed, frame=first_frame + f) feeds the networks), then infer_tensors on all n clouds - sliced by batch_size,
        so the networks see full batches instead of one frame's five clouds - and the identity for the detections without a cloud."""
        frames = list(frames)
        cls = np.concatenate([np.asarray(fr[3], dtype=np.int64).reshape(-1) for fr in frames]) if frames else np.zeros(0, dtype=np.int64)
        return self._infer_front_end(lambda fe: fe.device_clouds_frames([fr[:3] for fr in frames], seed, first_run=first_frame), cls)

    def evaluate(self, detect_result, out_dir=None, degree_thresholds=tuple(range(0, 46)), shift_thresholds=tuple(i / 2 for i in range(21)),
                 iou_thresholds=tuple(i / 100 for i in range(101)), pooling_mode="average", ranker="energy_ranker"):
        """inference_pose -> inference_energy -> evaluate (evaluation_single.py:356-544) on the reference's `detect_result` dict
        (img_path -> {'result', 'valid_pts', 'cat_id', 'valid_inst'}, what detect_mrcnn_genpose pickles): fills every valid
        instance's K hypotheses (ranked by energy, as pred_energy_batch stores them) and energies in place, then computes mAP
        with the reference's threshold grids.  Returns (iou_aps, pose_aps, iou_acc, pose_acc, store)."""
        from . import evaluation
        if self.ranker == "likelihood":
            if ranker == "energy_ranker":
                ranker = "likelihood_ranker"  # the array stored as 'energy' holds the log-likelihoods: ranked as it stands
        elif self.ranker == "consensus":
            if ranker == "energy_ranker":
                ranker = "consensus_ranker"  # compute_mAP scores the stored hypotheses itself, the symmetric categories by their y axis
        elif self.energy_agent is None:
            raise ValueError("evaluation needs the energy agent (hypotheses are ranked by energy)")
        store = evaluation.DetectionResults(detect_result, self.repeat_num)
        for cat in store.by_category:
            for sl, pts in store.batches(cat, self.batch_size):
                res = self.infer(pts, sym=np.full(len(pts), cat in evaluation._Y_SYMMETRIC)) if self.ranker == "consensus" else self.infer(pts)
                sorted_energy = -np.sort(-res["energy"], axis=1)  # sort_poses_by_energy's second output (reward.py:146-147)
                store.write(cat, sl, res["sorted_RTs"], sorted_energy)
        maps = evaluation.compute_mAP(store.results(), out_dir, list(degree_thresholds), list(shift_thresholds), list(iou_thresholds),
                                      iou_pose_thres=0.1, use_matches_for_pose=True, repeat_num=self.repeat_num, pooling_mode=pooling_mode,
                                      ratio=self.ratio, ranker=ranker)
        return maps + (store,)


# ------------------------------------------------------------------ tracking
def _unit(q):
    return q / q.norm(dim=-1, keepdim=True)


def add_noise_to_RT(RT, r=5.0, t=0.03, draws=None):
    """Initial-pose jitter of the tracking runner (utils/tracking_utils.py:37-101, 'normal' mode): rotate by
    |N(0,1)|*r degrees about a random axis orthogonal (in quaternion space) to the current rotation and shift by
    N(0,1)*t metres along a random direction.  `draws` (tests): the four standard-normal tensors in call order
    (theta [B], quaternion [B,4], shift norm [B], direction [B,3])."""
    B = RT.shape[0]
    if draws is None:
        draws = [torch.randn(B), torch.randn(B, 4), torch.randn(B), torch.randn(B, 3)]
    d_theta, d_q, d_norm, d_dir = [d.to(RT) for d in draws]
    Rm = RT[:, :3, :3]
    theta = (d_theta.abs() * (r / 180 * math.pi)).unsqueeze(-1)
    tr = torch.clamp(1 + Rm[:, 0, 0] + Rm[:, 1, 1] + Rm[:, 2, 2], min=0.0)
    rr = torch.sqrt(tr)
    s = 1.0 / (2 * rr + 1e-7)
    q = _unit(torch.stack((0.5 * rr, (Rm[:, 2, 1] - Rm[:, 1, 2]) * s, (Rm[:, 0, 2] - Rm[:, 2, 0]) * s, (Rm[:, 1, 0] - Rm[:, 0, 1]) * s), dim=-1))
    nq = _unit(d_q)
    q_orth = _unit(nq - q * torch.sum(q * nq, dim=-1, keepdim=True))
    jq = q * torch.cos(theta / 2) + q_orth * torch.sin(theta / 2)
    w, x, y, z = torch.unbind(jq, dim=-1)
    new_R = torch.stack((1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w,
                         2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w,
                         2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y), dim=-1).reshape(B, 3, 3)
    out = RT.clone()
    out[:, :3, :3] = new_R
    direction = d_dir / torch.clamp(d_dir.norm(dim=-1, keepdim=True), min=1e-9)
    out[:, :3, 3] = RT[:, :3, 3] + direction * (d_norm * t).unsqueeze(-1)
    return out


class _FrameGraphs:
    """hipGraphs of the launch sequences of a tracking frame that need no host decision, keyed by the clouds' shape:
      A   clouds [n,1024,3] -> centres, the SCORE model's per-cloud embedding: grouping (furthest point sampling with its deeper levels on a
          side branch under level 0, ball queries) once, the score model's encoder, its cloud embedding;
      A'  the ENERGY model's encoder on the same centres and neighbourhoods + its cloud embedding.  Nothing before the ranking needs it,
          and the adaptive solve of a frame occupies 10-19 of the 256 CUs: A' is replayed on a side stream and runs UNDERNEATH the solve;
      B   candidates [n,K,9] -> energies -> ranking -> top-`sel` aggregation -> 4x4 poses (energy evaluation, gp_rank_aggregate and
          the small conversions); waits for A'.
    Between A and B sits the adaptive ODE solve, whose attempts are graph replays of their own.  A 5-object frame is then A + the
    solve's replay(s) + B instead of ~70 individually launched kernels.  Inputs are copied into static buffers, outputs are static
    tensors that the NEXT frame of the same shape overwrites (callers that keep them clone).

    enet None (a tracker on one network, FixedStepTracker): A alone - one plain encoder pass, no side stream (ev_e is None), cvec_e is
    None; with T_energy, `snet` is an ENERGY network that also ranks, on the embedding A leaves."""

    def __init__(self, snet, enet=None, K=None, sel=None, T_energy=1e-5):
        """T_energy: the time the ranking network (enet, else snet) is evaluated at; None: nothing ranks by energy."""
        from .sde import SIGMA_MAX, SIGMA_MIN
        self.snet, self.enet, self.K, self.sel = snet, enet, K, sel
        self.nets = (snet,) if enet is None else (snet, enet)
        for net in self.nets:
            net.pointnet2_encoder("the frame-graph runner")  # refuses an agent whose features are not the PointNet++ encoder's alone
        dev = snet.device
        if T_energy is not None:
            t = torch.full((1,), float(T_energy), device=dev)
            self.tvec_e = self.nets[-1].pose_score_net.time_embed(t)[0].contiguous()
            self.sigma_e = (SIGMA_MIN * (SIGMA_MAX / SIGMA_MIN) ** t).contiguous()
        # the replays write into encoder workspaces of their own: no ticket of the agent path ever points at them
        self.SLOT = "frame-graphs" if enet is not None else "fixed-step-tracker"
        self.share = enet is not None and snet.pts_encoder.grouping_key() == enet.pts_encoder.grouping_key()
        self.side = self.ev_a = self.ev_e = None
        if enet is not None:
            self.side = torch.cuda.Stream(dev)
            self.ev_a, self.ev_e = torch.cuda.Event(), torch.cuda.Event()
        # per object count of a frame: bounded (lru.py); a dropped entry gives its encoder workspaces back to their eviction order
        self._a = ShapeCache(self.MAX_SHAPES, on_evict=release)
        self._b = ShapeCache(self.MAX_SHAPES)

    MAX_SHAPES = 8

    def _score_body(self, pts):
        enc_s = self.snet.pts_encoder
        # (deferred join: the deeper sampling levels run on a side branch of the graph underneath the level-0 set abstraction)
        grouping = enc_s.prepare_grouping(pts, slot=self.SLOT, defer_join=True) if self.share else None
        cvec_s = self.snet.pose_score_net.cloud_embed(enc_s.forward(pts, slot=self.SLOT, grouping=grouping))
        return grouping, pts.mean(dim=1), cvec_s

    def _energy_body(self, pts, grouping):
        return self.enet.pose_score_net.cloud_embed(self.enet.pts_encoder.forward(pts, slot=self.SLOT, grouping=grouping))

    def embed(self, pts):
        """-> (centre [n,3], cvec of the score model [n,768], cvec of the energy model [n,768]); the energy model's embedding is still
        being computed on the side stream when this returns - rank() waits for it."""
        key = (tuple(pts.shape), pts.dtype)
        ent = self._a.get(key)
        if ent is None:
            ent = self._a[key] = self._capture_embed(pts.clone())
        if self.enet is None:
            return ent.replay(pts)
        cur = torch.cuda.current_stream(pts.device)
        cur.wait_event(self.ev_e)  # the previous frame's A' (side stream) has finished reading `buf`, which is about to change
        ent.replay(pts)
        self.ev_a.record(cur)
        with torch.cuda.stream(self.side):
            self.side.wait_event(self.ev_a)
            ent.extra["side"].replay()
            self.ev_e.record(self.side)
        return ent.outs

    def _capture_embed(self, buf):
        """One entry for A and A': `outs` = (centre, cvec_s, cvec_e or None), A' as extra['side']."""
        n, N, two = int(buf.shape[0]), int(buf.shape[1]), self.enet is not None

        def warm():  # outside capture: workspaces, kernel attributes
            grouping = self._score_body(buf)[0]
            if two:
                self._energy_body(buf, grouping)
        # the replays write into encoder workspaces that were allocated outside the captures: pinned - around BOTH captures and before the
        # first, so that none of them can be re-allocated inside one and a failure in either gives every pin back - for as long as these
        # graphs live
        with holding([lambda net=net: net.pts_encoder.pin_workspaces(n, N, self.SLOT) for net in self.nets]) as pinned:
            ent = capture(lambda: self._score_body(buf), bufs=(buf,), warmup=warm)
            grouping, centre, cvec_s = ent.outs
            side = capture(lambda: self._energy_body(buf, grouping), stream=self.side) if two else None
        ent.outs, ent.pinned, ent.extra["side"] = (centre, cvec_s, side.outs if two else None), pinned, side
        return ent

    def _rank_body(self, pred, centre, cvec_e):
        n, K = pred.shape[0], self.K
        pose = pred.to(torch.float32, copy=True)
        pose[:, :, 6:] -= centre.unsqueeze(1)  # posenet_agent.py:516: translations relative to the cloud centre
        energy = self.enet.pose_score_net.evaluate(cvec_e, K, pose.reshape(n * K, 9), self.tvec_e, self.sigma_e, "energy").reshape(n, K, 2)
        r = reward.rank_aggregate(pred, energy, selected_num=self.sel, with_rt=True)  # ranking, aggregation and both 4x4 forms: one launch
        return energy, r["sorted_RTs"], r["avg_RT"]

    def rank(self, pred, centre, cvec_e):
        """pred [n,K,9] f64 -> (energy [n,K,2], sorted_RTs [n,K,4,4], average_sRT [n,4,4])"""
        key = (tuple(pred.shape), pred.dtype)
        ent = self._b.get(key)
        torch.cuda.current_stream(pred.device).wait_event(self.ev_e)  # the energy model's embedding (side stream, under the solve)
        if ent is None:
            bufs = (pred.clone(), centre.clone(), cvec_e.clone())
            ent = self._b[key] = capture(lambda: self._rank_body(*bufs), bufs=bufs, warmup=True)
        return ent.replay(pred, centre, cvec_e)


class TrackingRunner:
    """Frame-by-frame tracking with warm-started candidates (main_tracking, evaluation_tracking.py:262-337):
    every instance of a frame forms one batch; the initial pose of an object is the previous frame's aggregated
    sRT for the same `model_name`, else a jittered ground-truth pose; the ODE sampler starts at T0 = 0.15 from
    init_x + prior(T0) (samplers.py:180).

    use_graphs (default): the launch sequences around the adaptive solve are replayed as two hipGraphs per object count
    (_FrameGraphs) - same kernels, same results as the agents' pred_func -> get_energy -> rank_aggregate called one after the other
    (use_graphs=False), a third fewer microseconds per frame at tracking sizes, where launch overhead dominates."""

    def __init__(self, score_agent, energy_agent, repeat_num=50, T0=0.15, ratio=0.6, use_graphs=True, ranker="energy"):
        if ranker != "energy":
            raise NotImplementedError(f"TrackingRunner(ranker={ranker!r}): tracking ranks by the energy model only; the likelihood ranker "
                                      "(SingleFrameRunner(ranker='likelihood')) is not wired into the frame loop")
        self.score_agent, self.energy_agent = score_agent, energy_agent
        self.repeat_num, self.T0, self.ratio = repeat_num, T0, ratio
        self.buffer = {"model_name": [], "pred_sRT": None}
        self.use_graphs = use_graphs
        if use_graphs:  # the frame graphs drive the PointNet++ encoder's stages themselves: refused here, not at the first frame
            if score_agent.cfg.sampler_mode[0] in ("heun", "dpm2m"):
                raise NotImplementedError("TrackingRunner(use_graphs=True) builds its frame graphs around the adaptive ODE solve and does not serve "
                                          f"sampler_mode ['{score_agent.cfg.sampler_mode[0]}']: use use_graphs=False (the agent's pred_func)")
            for a in (score_agent, energy_agent):
                a.net.pointnet2_encoder("TrackingRunner(use_graphs=True)")
        self._graphs = None

    def reset(self):
        self.buffer = {"model_name": [], "pred_sRT": None}

    def step(self, pts, model_names, gt_RT, noise_draws=None):
        """pts [n,1024,3] device tensor; gt_RT [n,4,4] (used only for objects not seen in the previous frame)."""
        pts = pts.float()
        dev = pts.device
        K = self.repeat_num
        sel = max(1, int(self.ratio * K))
        # (a coupled agent - its batch sharded over a process group - keeps the agent path: the frame graphs build an uncoupled solver)
        graphs = self.use_graphs and self.score_agent.cfg.sampler_mode[0] == "ode" and getattr(self.score_agent.net, "coupling_group", None) is None
        if graphs:
            net = self.score_agent.net
            net._need_weights()
            self.energy_agent.net._need_weights()
            if self._graphs is None:
                self._graphs = _FrameGraphs(net, self.energy_agent.net, K, sel)
            # graph A first: the clouds' centres come out of it (the mean the sample dict would hold, evaluation_tracking.py:306-311)
            centre, cvec_s, cvec_e = self._graphs.embed(pts)
            sample = None
        else:
            sample = make_batch_sample(pts)
            centre = sample["pts_center"]
        with _one_cpu_thread():
            noised = add_noise_to_RT(gt_RT.float().cpu(), draws=noise_draws)  # drawn every frame (:302), whether or not it is used
        if (self.buffer["pred_sRT"] is not None and list(model_names) == self.buffer["model_name"]
                and len(set(model_names)) == len(model_names)):
            # every object continues from the previous frame: nothing to upload, one tensor.  (Unique names only: the reference looks a
            # name up with list.index (evaluation_tracking.py:303-307) - two objects with the SAME name both get the first one's pose,
            # which the general branch below reproduces.)
            init_sRT = self.buffer["pred_sRT"].float()
        else:
            init_sRT = noised.to(dev)
            for i, name in enumerate(model_names):
                if name in self.buffer["model_name"]:
                    init_sRT[i] = self.buffer["pred_sRT"][self.buffer["model_name"].index(name)]
        init_x = torch.cat([init_sRT[:, :3, 0], init_sRT[:, :3, 1], init_sRT[:, :3, 3] - centre], dim=1)  # [R[:,0], R[:,1], t - centre]
        if graphs:
            from .samplers import ODESampler
            n = pts.shape[0]
            prior = net._prior_to_device((n * K, 9), T=self.T0)
            x0 = (prior.view(n, K, 9) + init_x.float().unsqueeze(1)).view(n * K, 9)  # samplers.py:180: init_x repeated K times + prior
            trunk = getattr(net.cfg, "ode_trunk", None)
            key = ("ode", n, K, None, trunk)
            smp = net._samplers.get(key)
            if smp is None:
                smp = net._samplers[key] = ODESampler(net.pose_score_net, n, K, net.device, trunk=trunk)
            net.last_sampler = smp
            _, x = smp.run(cvec_s, centre, x0, self.T0, num_steps=net.cfg.sampling_steps, eps=net.sampling_eps)
            pred = x.reshape(n, K, 9)
            energy, sorted_RTs, average_sRT = self._graphs.rank(pred, centre, cvec_e)
            energy, sorted_RTs, average_sRT = energy.clone(), sorted_RTs.clone(), average_sRT.clone()
        else:
            pred = self.score_agent.pred_func(data=sample, repeat_num=K, save_path=None, init_x=init_x.float(), T0=self.T0)
            energy = self.energy_agent.get_energy(data=sample, pose_samples=pred, T=1e-5)
            r = reward.rank_aggregate(pred, energy, selected_num=sel, with_rt=True)
            average_sRT, sorted_RTs = r["avg_RT"], r["sorted_RTs"]
        self.buffer = {"model_name": list(model_names), "pred_sRT": average_sRT}
        # (the caller gets its own copy of the aggregated poses: the buffer's tensor is the next frame's warm start)
        return {"init_x": init_x, "pred_pose": pred, "energy": energy, "sorted_RTs": sorted_RTs, "average_sRT": average_sRT.clone()}


class MultiSequenceTracker:
    """Tracking (main_tracking, evaluation_tracking.py:262-337) for SEVERAL sequences at once - BASELINE configs[4]: a frame of one
    sequence is a tiny batch (4-6 objects x 50 candidates), so the frames that different sequences are at share every launch:
    one encoder pass over all their clouds, one device-resident RK45 solve in which every sequence's frame is a group with
    its own step control (gp_rk45_phase_ragged - exactly what a per-sequence cond_ode_sampler call does), one energy pass, one
    ranking launch.  Per sequence the semantics are TrackingRunner's: warm start from the previous frame's aggregated pose
    of the same `model_name`, else the jittered ground truth; T0 = 0.15."""

    def __init__(self, score_agent, energy_agent, n_sequences, repeat_num=50, T0=0.15, ratio=0.6, max_objects_per_frame=8):
        self.score_agent, self.energy_agent = score_agent, energy_agent
        self.repeat_num, self.T0, self.ratio = repeat_num, T0, ratio
        self.buffers = [{"model_name": [], "pred_sRT": None} for _ in range(n_sequences)]
        # one solver sized for the capacity; the group tables are re-filled every step, so frames whose object counts change
        # keep replaying the same captured graphs
        self.cap_groups, self.cap_clouds = n_sequences, n_sequences * max_objects_per_frame
        self._sampler = None
        self._prev = None  # (live sequences, their aggregated poses [objects,4,4] in step order) of the previous step
        self.one_tensor_warm_starts = 0  # steps whose initial poses were the previous step's aggregated poses as they stood

    def reset(self, seq=None):
        for i in (range(len(self.buffers)) if seq is None else [seq]):
            self.buffers[i] = {"model_name": [], "pred_sRT": None}
        self._prev = None

    def step(self, frames, noise_draws=None, prior=None):
        """frames: one (pts [n_i,1024,3] device, model_names [n_i], gt_RT [n_i,4,4]) per sequence (None = the sequence has no
        frame this step).  Returns one TrackingRunner-style dict per sequence (None where there was no frame).
        prior (tests): per sequence, the prior draw [n_i*K,9] exactly as `prior_fn((n_i*K, 9), T=T0)` returns it (already scaled by
        sigma(T0)) - it stands in for prior_fn, unlike the `prior_noise` of the pipeline predictors (standard-normal draws).
        The returned tensors are slices of the step's own result tensors; `average_sRT` is a copy (the tracker keeps the original as the
        next step's warm start, so an in-place edit by the caller - a unit conversion, a scale - cannot reach it)."""
        from .samplers import ODESampler
        net = self.score_agent.net
        net._need_weights()
        K = self.repeat_num
        live = [i for i, f in enumerate(frames) if f is not None and f[0].shape[0] > 0]
        out = [None] * len(frames)
        if not live:
            return out
        dev = frames[live[0]][0].device
        counts = [int(frames[i][0].shape[0]) for i in live]
        pts = torch.cat([frames[i][0].float() for i in live], dim=0)
        centre = pts.mean(dim=1)
        # initial poses: jittered ground truth for every object (drawn every frame, evaluation_tracking.py:302) in ONE host call and
        # one upload, then the warm starts gathered from the previous frames' aggregated poses in one indexed copy
        gt_all = torch.cat([frames[i][2].float().cpu() for i in live], dim=0)
        draws_all = None if noise_draws is None else [torch.cat([noise_draws[i][d] for i in live], dim=0) for d in range(4)]
        with _one_cpu_thread():
            noised = add_noise_to_RT(gt_all, draws=draws_all)  # drawn every frame (evaluation_tracking.py:302), whether or not it is used
        if (self._prev is not None and self._prev[0] == live
                and all(list(frames[i][1]) == self.buffers[i]["model_name"] and len(set(frames[i][1])) == len(frames[i][1]) for i in live)):
            # (unique names per frame only: duplicates go through list.index below, first match, as evaluation_tracking.py:303-307)
            # every object of every sequence continues from the previous step, in the same order: the previous aggregated poses ARE the
            # initial poses - nothing to upload, no index tensors (their pageable host-to-device copies wait for the stream)
            init_sRT = self._prev[1]
            self.one_tensor_warm_starts += 1
        else:
            init_sRT = noised.to(dev)
            prev, src, dst, off, row = [], [], [], 0, 0
            for q, i in enumerate(live):
                buf = self.buffers[i]
                if buf["pred_sRT"] is not None:
                    for j, name in enumerate(frames[i][1]):
                        if name in buf["model_name"]:
                            src.append(off + buf["model_name"].index(name))
                            dst.append(row + j)
                    prev.append(buf["pred_sRT"])
                    off += buf["pred_sRT"].shape[0]
                row += counts[q]
            if src:
                init_sRT[torch.as_tensor(dst, device=dev)] = torch.cat(prev, dim=0)[torch.as_tensor(src, device=dev)].to(init_sRT.dtype)
        init_x = torch.cat([init_sRT[:, :3, 0], init_sRT[:, :3, 1], init_sRT[:, :3, 3] - centre], dim=1)  # [R[:,0], R[:,1], t - centre]
        # ---- score model: encoder -> warm-started ODE, one group per sequence
        shared = {"pts": pts, "pts_center": centre}
        # (launch by launch: the cloud count of a multi-sequence step changes from frame to frame and the pass is not launch-bound here)
        feat = net.extract_pts_feature(shared, use_graph=False)  # leaves the grouping ticket for the energy agent
        cvec = net.pose_score_net.cloud_embed(feat)
        B = pts.shape[0]
        if prior is None:
            pr = net._prior_to_device((B * K, 9), T=self.T0)
        else:
            pr = torch.cat([prior[i].reshape(-1, 9) for i in live], dim=0).to(dev).float()
        x0 = (pr.view(B, K, 9) + init_x.float().unsqueeze(1)).view(B * K, 9)  # samplers.py:180: init_x repeated K times + prior
        if B > self.cap_clouds:
            raise ValueError(f"{B} objects in this step exceed the capacity {self.cap_clouds} (n_sequences x max_objects_per_frame)")
        smp = self._sampler
        if smp is None:
            per = self.cap_clouds // self.cap_groups
            smp = self._sampler = ODESampler(net.pose_score_net, self.cap_clouds, K, dev, group_clouds=[per] * self.cap_groups)
        smp.set_groups(counts)
        _, x = smp.run(cvec, centre, x0, self.T0, num_steps=net.cfg.sampling_steps, eps=net.sampling_eps)
        pred = x.reshape(B, K, 9)
        # ---- energy model + ranking + aggregation for all clouds at once (row / cloud local)
        energy = self.energy_agent.get_energy(data=shared, pose_samples=pred, T=1e-5)
        sel = max(1, int(self.ratio * K))
        r = reward.rank_aggregate(pred, energy, selected_num=sel, with_rt=True)
        average_sRT, sorted_RTs = r["avg_RT"], r["sorted_RTs"]
        lo = 0
        for_caller = average_sRT.clone()  # one small device-side copy, no synchronisation
        for q, i in enumerate(live):
            sl = slice(lo, lo + counts[q])
            lo += counts[q]
            self.buffers[i] = {"model_name": list(frames[i][1]), "pred_sRT": average_sRT[sl]}  # (views of this step's own tensor)
            out[i] = {"init_x": init_x[sl], "pred_pose": pred[sl], "energy": energy[sl], "sorted_RTs": sorted_RTs[sl], "average_sRT": for_caller[sl],
                      "nfev": int(smp.group_stats[q]["nfev"])}
        self._prev = (live, average_sRT)
        return out


class FixedStepTracker:
    """Tracking (main_tracking, evaluation_tracking.py:262-337) on the fixed-step Heun solver, with the frame resident on the device.  The
    solve has a fixed number of evaluations, so nothing between the clouds and the aggregated 4x4 poses needs a host decision: a step whose
    frame layout was seen before copies the clouds into a static buffer, writes the seed state through a pinned block in stream order and
    replays captured graphs - the encoders and cloud embeddings (_FrameGraphs' A, with A' on its side stream; one graph without an energy
    agent), then ONE graph holding the warm start with the prior drawn on the device (gp_track_warm_start: no host draw, no upload), the
    Heun solve (samplers.HeunSampler as a chain of 2 N + 2 launches or as one launch), the ranker and gp_rank_aggregate_rt.  No per-kernel
    launch, no read-back: last_stats['replays'] <= 3.

    step(frames): one (pts [n_i,1024,3], model_names, gt_RT [n_i,4,4]) per sequence, None where a sequence has no frame - one sequence is
    the list of one.  The live sequences' clouds share every launch; every stage is row-local or cloud-local and the prior's draw of a
    candidate is a function of (seed, sequence, frame of the sequence, object, candidate) - global row (sequence * max_objects_per_frame +
    object) * K + k, the sequence's own frame count as the run word - so a sequence's result does not depend on what shares the step.
    Returns one dict per sequence (None where there was no frame): init_x, pred_pose [n,K,9] f32, energy [n,K,2], sorted_RTs [n,K,4,4]
    f64, average_sRT [n,4,4] and nfev; all of them the caller's own copies.

    Warm start: the reference's semantics - an object continues from the previous frame's aggregated sRT of the same model_name (first
    match of list.index, duplicates included), else from a jittered gt_RT.  The jitter (add_noise_to_RT) is drawn on the host ONLY in a
    step that has an object without a predecessor, from a generator keyed by (seed, sequence, frame); the reference draws it every frame
    on the global generator - this tracker claims NO random-number parity with the reference or with TrackingRunner.  In steady state the
    source table is cached and nothing is uploaded but the seed state.

    ranker: 'energy' - the energy agent's two energies at T = 1e-5; 'likelihood' - the score agent's own exact-divergence log-likelihood by
    samplers.HeunLikelihood (cfg.likelihood_steps, else the tracker's steps; cfg.likelihood_grid) in both columns, cast to float32 as
    SingleFrameRunner does: tracking from a score checkpoint alone; 'consensus' - no ranking network either: the candidates' mutual
    agreement, scored, ranked and aggregated by ONE launch (gp_consensus_rank_aggregate_rt) in place of the likelihood solve and
    gp_rank_aggregate_rt - the score agent's embed graph and the frame's graph, last_stats['replays'] == 2.
    symmetric (ranker 'consensus'): callable model_name -> bool, True for objects symmetric about their y axis (their candidates are compared
    by that axis alone); None: no object is.  The flags are uploaded only in a step whose names differ from the previous step's.
    launches: 'single' / 'chain' force the solve's form; None takes 'single' below SINGLE_MAX_ROWS rows where the plan is a tile plan.
    solver: 'heun' (default) or 'dpm2m' - the same frame with samplers.Dpm2mSampler's solve (steps + 1 evaluations instead of 2 steps + 1)
    in HeunSampler's place; everything around the solve is unchanged.
    sample_from: 'score' (default) or 'energy' (ours; opt-in) - tracking from an ENERGY checkpoint alone: score_agent may be None, the solve
    runs on the energy agent's network with the energy model's score inside the kernels (samplers.HeunSampler / Dpm2mSampler(model='energy'))
    and ranker 'energy' evaluates the same network on the same cloud embedding - one encoder graph (no side stream) and the frame's graph,
    last_stats['replays'] == 2.  ranker 'energy' or 'consensus'; 'likelihood' is refused (likelihoods come from the score model).
    launches=None keeps the chain here: the energy model's one-launch solve measured slower than its chain (profiles/fixed_step_energy.txt).
    init: 'gt' (default) - the reference's evaluation protocol as above: an object without a predecessor starts from a jittered gt_RT.
    'prior' (ours; opt-in) - the tracker ACQUIRES such objects itself and needs no ground truth: frames[i][2] is ignored and may be None,
    nothing is drawn on the host.  Objects without a predecessor form schedule class 1 and start from the pure prior sigma(acquire_T0) z
    (cond_ode_sampler with init_x = None, samplers.py:180); the tracked ones are class 0 at T0; both run the same N steps in the same
    launches (gp_track_start_classes makes the class table on the device, samplers.HeunSampler / Dpm2mSampler(classes=2) solve).  The graph
    key stays (sequence, object count): a frame in which an object enters, leaves or is re-acquired after reset() captures nothing new.
    The class-aware solve runs in every frame of this mode; init_x of an acquired object is a zero row, last_stats['acquired'] counts them.
    Score model only (sample_from='energy' is refused)."""

    RANKERS = ("energy", "likelihood", "consensus")
    INITS = ("gt", "prior")
    SOLVERS = ("heun", "dpm2m")
    SAMPLE_FROM = ("score", "energy")
    LAUNCHES = (None, "single", "chain")
    # rows below which launches=None takes the one-launch solve.  profiles/fixed_step_tracking.txt: its median lay below the chain's minimum
    # at 250, 800 and 3 200 rows (16-row tiles, 1.09x) and above it at 12 800 rows (64-row tiles, 0.97x); nothing was measured in between
    SINGLE_MAX_ROWS = 3201
    MAX_SHAPES = 8
    RING = 4  # pinned blocks in rotation: the host rewrites one only after the copy issued four steps earlier has completed

    def __init__(self, score_agent, energy_agent=None, steps=8, repeat_num=50, T0=0.15, ratio=0.6, ranker="energy", seed=0, launches=None,
                 grid="geometric", max_objects_per_frame=8, solver="heun", symmetric=None, sample_from="score", init="gt", acquire_T0=0.55):
        from .samplers import HEUN_GRIDS
        if init not in self.INITS:
            raise ValueError(f"FixedStepTracker(init={init!r}): one of {self.INITS}")
        if init == "prior" and sample_from == "energy":
            raise ValueError("FixedStepTracker(init='prior', sample_from='energy'): schedule classes run on the score model; init='gt' or sample_from='score'")
        if init == "prior" and not 0.0 < float(acquire_T0) <= 1.0:
            raise ValueError(f"FixedStepTracker(acquire_T0={acquire_T0}): a diffusion time in (0, 1]")
        if solver not in self.SOLVERS:
            raise ValueError(f"FixedStepTracker(solver={solver!r}): one of {self.SOLVERS}")
        if sample_from not in self.SAMPLE_FROM:
            raise ValueError(f"FixedStepTracker(sample_from={sample_from!r}): one of {self.SAMPLE_FROM}")
        if sample_from == "energy":
            if ranker == "likelihood":
                raise ValueError("FixedStepTracker(sample_from='energy', ranker='likelihood'): likelihoods come from the score model; "
                                 "ranker 'energy' or 'consensus'")
            if energy_agent is None or energy_agent.cfg.posenet_mode != "energy":
                raise ValueError("FixedStepTracker(sample_from='energy') needs energy_agent with posenet_mode='energy'"
                                 + ("" if energy_agent is None else f", got {energy_agent.cfg.posenet_mode!r}"))
        elif score_agent.cfg.posenet_mode != "score":
            raise ValueError(f"FixedStepTracker: the score agent's posenet_mode is {score_agent.cfg.posenet_mode!r}, the Heun solver needs 'score' "
                             "(sample_from='energy' solves with the energy agent)")
        if ranker not in self.RANKERS:
            raise ValueError(f"FixedStepTracker(ranker={ranker!r}): one of {self.RANKERS}")
        if ranker == "energy" and energy_agent is None:
            raise ValueError("FixedStepTracker(ranker='energy') needs energy_agent (ranker='likelihood' tracks from the score agent alone)")
        if symmetric is not None and (ranker != "consensus" or not callable(symmetric)):
            raise ValueError("FixedStepTracker(symmetric=...): a callable model_name -> bool, for ranker='consensus'")
        if launches not in self.LAUNCHES:
            raise ValueError(f"FixedStepTracker(launches={launches!r}): one of {self.LAUNCHES}")
        if grid not in HEUN_GRIDS:
            raise ValueError(f"FixedStepTracker(grid={grid!r}): one of {HEUN_GRIDS}")
        if int(steps) < 1:
            raise ValueError(f"FixedStepTracker(steps={steps}): at least one step")
        if int(max_objects_per_frame) < 1 or int(repeat_num) < 1:
            raise ValueError(f"FixedStepTracker(max_objects_per_frame={max_objects_per_frame}, repeat_num={repeat_num}): at least one")
        # the agent whose network the solver runs on; sample_from 'energy': the energy agent, which then serves the energy ranker on the SAME
        # cloud embedding - one network, one encoder graph
        self.sample_from = sample_from
        self.sampling_agent = energy_agent if sample_from == "energy" else score_agent
        self._two_nets = ranker == "energy" and sample_from == "score"
        for a in (score_agent, energy_agent) if self._two_nets else (self.sampling_agent,):
            a.net.pointnet2_encoder("FixedStepTracker")  # refuses pts_encoder='pointnet_and_pointnet2': the graphs drive the PointNet++ stages
        if getattr(self.sampling_agent.net, "coupling_group", None) is not None:
            raise ValueError("FixedStepTracker: the score agent has a coupling_group (a batch sharded over a process group); the frame graphs build "
                             "an uncoupled solver - use the agent's pred_func")
        self.score_agent, self.energy_agent = score_agent, energy_agent if ranker == "energy" or sample_from == "energy" else None
        self.steps, self.repeat_num, self.T0, self.ratio = int(steps), int(repeat_num), float(T0), ratio
        self.ranker, self.seed, self.launches, self.grid = ranker, int(seed) % (1 << 64), launches, grid
        self.max_objects, self.solver, self.symmetric = int(max_objects_per_frame), solver, symmetric
        self.init, self.acquire_T0 = init, float(acquire_T0)
        self.buffers, self.frame_index = [], []
        self._embed = self._prev = None
        self._b = ShapeCache(self.MAX_SHAPES)
        self.captures = 0
        self.last_stats = {}

    def reset(self, seq=None):
        """Forget the previous poses (the next frame starts from jittered ground truth, or with init='prior' acquires every object again) and
        restart the frame count, of one sequence or all."""
        for i in (range(len(self.buffers)) if seq is None else [seq]):
            self.buffers[i], self.frame_index[i] = [], 0

    def pose_slots(self, seq, n):
        """The warm-start slots of sequence `seq`'s first n objects: a [n,4,4] f32 VIEW of the tensor the captured graphs read (where an
        object continues from) and write (its aggregated pose) - a caller that decides on the device whether an object keeps its new pose
        (DepthTracker: a lost object does not) overwrites it in stream order.  After the sequence's first step."""
        if self._prev is None or not 0 <= seq < len(self.buffers) or not 0 <= n <= self.max_objects:
            raise ValueError(f"pose_slots(seq={seq}, n={n}): a sequence that has had a step, at most max_objects_per_frame = {self.max_objects} objects")
        return self._prev[seq * self.max_objects: seq * self.max_objects + n]

    # ------------------------------------------------------------------ host side
    def _grow(self, nseq, dev):
        while len(self.buffers) < nseq:
            self.buffers.append([])
            self.frame_index.append(0)
        need = nseq * self.max_objects
        if self._prev is None or self._prev.shape[0] < need:
            # one slot per (sequence, object): the captured graphs read and write it, so a larger one means new graphs
            prev = torch.zeros(need, 4, 4, device=dev)
            if self._prev is not None:
                prev[: self._prev.shape[0]] = self._prev
            self._prev = prev
            self._b = ShapeCache(self.MAX_SHAPES)

    def _jitter(self, seq, gt_RT):
        g = torch.Generator().manual_seed((self.seed * 1000003 + seq * 7919 + self.frame_index[seq]) % (1 << 63))
        B = gt_RT.shape[0]
        draws = [torch.randn(B, generator=g), torch.randn(B, 4, generator=g), torch.randn(B, generator=g), torch.randn(B, 3, generator=g)]
        return add_noise_to_RT(gt_RT.float().cpu(), draws=draws)

    def _solve_form(self, rows, plan):
        if self.launches is not None:
            return self.launches
        if self.sample_from == "energy":
            # profiles/fixed_step_energy.txt: the energy model's one-launch solve is SLOWER than its chain at 250 and 3 200 rows
            # (chain / single 0.92 - 0.94x; an evaluation is a forward + backward pass of ~40 us, the launches between them are not what binds)
            return "chain"
        return "single" if plan != 128 and rows < self.SINGLE_MAX_ROWS else "chain"

    # ------------------------------------------------------------------ the frame's second graph
    def _body(self, ent):
        from ._lib import ptr, stream_ptr
        from .likelihood import global_prior_likelihood
        from .sde import SIGMA_MAX
        key, smp, K = ent["key"], ent["smp"], self.repeat_num
        _, cvec_s, cvec_e = ent["a_outs"]
        # the clouds' centres, reduced PER SEQUENCE: a reduction over the whole step's clouds may split its sums by the batch's shape, and a
        # sequence's result must not depend on what shares the step (graph A's own centres, taken over all clouds, are not used)
        lo, cen = 0, []
        for _, c in key:
            cen.append(torch.mean(ent["pts"][lo:lo + c][:, :, :3], dim=1))
            lo += c
        centre = smp.centre = torch.cat(cen, dim=0) if len(cen) > 1 else cen[0]
        n = centre.shape[0]
        # the poses the frame starts from (evaluation_tracking.py:302-310), for the caller; the kernel below forms them itself
        src = ent["src"].long()
        init_sRT = torch.where((src >= 0).view(n, 1, 1), self._prev.index_select(0, src.clamp(min=0)), ent["fallback"])
        init_x = torch.cat([init_sRT[:, :3, 0], init_sRT[:, :3, 1], init_sRT[:, :3, 3] - centre], dim=1)
        if self.init == "prior":  # an acquired object starts from the prior alone: a zero row
            init_x = torch.where((src >= 0).view(n, 1), init_x, torch.zeros_like(init_x))
        lo = 0
        for q, (_, c) in enumerate(key):  # one launch per sequence: its own row base and frame index
            if self.init == "prior":  # the start states and the solve's class table (class 1: acquired), no fallback pose
                _lib.call("gp_track_start_classes", c, K, ptr(ent["seed"][q]), ptr(smp.sched), smp.nlaunch * smp.SCHED_ROW, ptr(self._prev),
                          ptr(ent["src"][lo:lo + c]), None, ptr(centre[lo:lo + c]), ptr(smp.x[lo * K:(lo + c) * K]), ptr(smp.cls[lo:lo + c]), 1,
                          stream_ptr())
            else:
                _lib.call("gp_track_warm_start", c, K, ptr(ent["seed"][q]), ptr(smp.sched), ptr(self._prev), ptr(ent["src"][lo:lo + c]),
                          ptr(ent["fallback"][lo:lo + c]), ptr(centre[lo:lo + c]), ptr(smp.x[lo * K:(lo + c) * K]), stream_ptr())
            lo += c
        smp._launch_all()
        pred = smp.out.view(n, K, 9)
        if self.ranker == "consensus":  # score, ranking, aggregation and both 4x4 forms: one launch
            r = reward.consensus_rank_aggregate(pred, ent["sym"], selected_num=ent["sel"], with_rt=True)
            self._prev.index_copy_(0, ent["dst"], r["avg_RT"])
            return init_x, pred, r["energy"], r["sorted_RTs"], r["avg_RT"]
        pose = pred.clone()
        pose[:, :, 6:] -= centre.unsqueeze(1)  # posenet_agent.py:516: translations relative to the cloud centre
        if self.ranker == "energy":
            if not self._two_nets:  # sample_from 'energy': the network that drew the candidates ranks them, on the embedding the solve used
                cvec_e = cvec_s
            energy = self.energy_agent.net.pose_score_net.evaluate(cvec_e, K, pose.reshape(n * K, 9), self._embed.tvec_e, self._embed.sigma_e,
                                                                   "energy").reshape(n, K, 2)
        else:
            lk = ent["lik"]
            lk.x.copy_(pose.reshape(n * K, 9))
            lk._launch_all()
            ll = (global_prior_likelihood(lk.z.double(), SIGMA_MAX) + lk.logp) / math.log(2)
            ll32 = ll.float().view(n, K)
            energy = torch.stack([ll32, ll32], dim=-1).contiguous()
        r = reward.rank_aggregate(pred, energy, selected_num=ent["sel"], with_rt=True)
        self._prev.index_copy_(0, ent["dst"], r["avg_RT"])
        return init_x, pred, energy, r["sorted_RTs"], r["avg_RT"]

    def _capture(self, key, a_outs, pts):
        from .samplers import Dpm2mSampler, HeunLikelihood, HeunSampler
        net = self.sampling_agent.net
        K = self.repeat_num
        n, dev = sum(c for _, c in key), pts.device
        Solver = Dpm2mSampler if self.solver == "dpm2m" else HeunSampler
        kw = dict(grid=self.grid, use_graph=False, model=self.sample_from)
        if self.init == "prior":
            kw["classes"] = 2  # class 0: tracked at T0; class 1: acquired at acquire_T0
        probe = Solver(net.pose_score_net, n, K, self.steps, dev, **kw)
        form = self._solve_form(n * K, probe.plan)
        smp = probe if form == "chain" else Solver(net.pose_score_net, n, K, self.steps, dev, launches=form, **kw)
        smp.cvec = a_outs[1]  # graph A's static output: nothing is copied
        ent = {"key": key, "smp": smp, "a_outs": a_outs, "sel": max(1, int(self.ratio * K)),
               "src": torch.full((n,), -1, dtype=torch.int32, device=dev), "fallback": torch.zeros(n, 4, 4, device=dev),
               "seed": torch.zeros(len(key), 8, dtype=torch.int32, device=dev), "pts": pts.clone(),
               "dst": torch.tensor([i * self.max_objects + j for i, c in key for j in range(c)], dtype=torch.int64, device=dev),
               "src_host": None, "ring": UploadRing(self.RING)}
        smp._write_schedule((self.T0, self.acquire_T0) if self.init == "prior" else self.T0, net.sampling_eps)
        if self.ranker == "consensus":  # the symmetry flags: static, read by the captured launch; NULL (no object symmetric) without `symmetric`
            ent["sym"] = ent["sym_host"] = None
            if self.symmetric is not None:
                ent["sym"], ent["sym_host"] = torch.zeros(n, dtype=torch.int8, device=dev), [0] * n
        if self.ranker == "likelihood":
            lsteps = getattr(net.cfg, "likelihood_steps", None) or self.steps
            lk = ent["lik"] = HeunLikelihood(net.pose_score_net, n, K, dev, int(lsteps), grid=getattr(net.cfg, "likelihood_grid", "geometric"), use_graph=False)
            lk.cvec = a_outs[1]
            lk._write_schedule(net.sampling_eps, 1.0)
        keep = self._prev.clone()

        def warm():  # outside capture: kernel attributes, the allocator's blocks
            self._body(ent)
            self._prev.copy_(keep)  # (the warm-up ran on placeholders and wrote its poses into the slots)
        # (no `bufs`: step() fills the static inputs itself - the clouds ahead of the pinned uploads, the tables only when they change)
        captured = capture(lambda: self._body(ent), warmup=warm, extra=ent)
        self.captures += 1
        return captured

    def step(self, frames):
        net = self.sampling_agent.net
        K = self.repeat_num
        live = [i for i, f in enumerate(frames) if f is not None and f[0].shape[0] > 0]
        out = [None] * len(frames)
        if not live:
            return out
        net._need_weights()
        for i in live:
            if frames[i][0].shape[0] > self.max_objects or len(frames[i][1]) != frames[i][0].shape[0]:
                raise ValueError(f"sequence {i}: {frames[i][0].shape[0]} objects / {len(frames[i][1])} names; at most max_objects_per_frame = {self.max_objects}")
        dev = frames[live[0]][0].device
        self._grow(len(frames), dev)
        if self._embed is None:
            if self._two_nets:
                self.energy_agent.net._need_weights()
            # one network: the score model's, or (sample_from 'energy') the energy model's, which then ranks on the same embedding
            self._embed = _FrameGraphs(net, self.energy_agent.net if self._two_nets else None, K, max(1, int(self.ratio * K)),
                                       T_energy=1e-5 if self.ranker == "energy" else None)
        key = tuple((i, int(frames[i][0].shape[0])) for i in live)
        pts = torch.cat([frames[i][0].float() for i in live], dim=0)
        a_outs = self._embed.embed(pts)
        replays = 2 if self._two_nets else 1
        captured = self._b.get(key)
        if captured is None or captured.extra["a_outs"][1] is not a_outs[1]:  # (graph A of this cloud count was dropped and captured again: new static tensors)
            captured = self._b[key] = self._capture(key, a_outs, pts)
        ent = captured.extra  # the sampler, the static tables, their host mirrors and the ring of pinned blocks
        # ---- warm-start table: where every object continues from
        src, fresh = [], False
        for i in live:
            names = self.buffers[i]
            for name in frames[i][1]:
                src.append(i * self.max_objects + names.index(name) if name in names else -1)
                fresh = fresh or (src[-1] < 0 and self.init == "gt")  # init 'prior': no fallback pose, nothing drawn or uploaded for it
        ent["pts"].copy_(pts)
        ring = ent["ring"]
        ring.advance()  # (each block is rewritten RING steps after the copy out of it was issued: long completed)
        with _one_cpu_thread():
            if fresh:
                ring.send("fallback", ent["fallback"], lambda h: h.copy_(torch.cat([self._jitter(i, frames[i][2]) for i in live], dim=0)))
            uploaded = src != ent["src_host"]
            if uploaded:
                ring.send("src", ent["src"], lambda h: h.copy_(torch.tensor(src, dtype=torch.int32)))
                ent["src_host"] = src
            if self.symmetric is not None:
                sym = [int(bool(self.symmetric(name))) for i in live for name in frames[i][1]]
                if sym != ent["sym_host"]:
                    ring.send("sym", ent["sym"], lambda h: h.copy_(torch.tensor(sym, dtype=torch.int8)))
                    ent["sym_host"] = sym
            words = np.stack([_lib.seed_words(self.seed, self.frame_index[i] % (1 << 32), i * self.max_objects * K) for i in live])
            ring.send("seed", ent["seed"], lambda h: h.copy_(torch.from_numpy(words.view(np.int32))))
        if self._two_nets:
            torch.cuda.current_stream(dev).wait_event(self._embed.ev_e)  # the energy model's embedding (side stream)
        replays += 1
        init_x, pred, energy, sorted_RTs, average_sRT = (t.clone() for t in captured.replay())
        smp = ent["smp"]
        self.last_stats = {"replays": replays, "captures": self.captures, "launches": smp.launches, "kernel": smp.kernel_name, "plan": smp.plan,
                           "nfev": smp.nlaunch - 1, "rows": pts.shape[0] * K, "uploaded_src": uploaded, "uploaded_fallback": fresh}
        if self.init == "prior":
            self.last_stats["acquired"] = sum(1 for v in src if v < 0)
        lo = 0
        for i in live:
            c = int(frames[i][0].shape[0])
            sl = slice(lo, lo + c)
            lo += c
            self.buffers[i] = list(frames[i][1])
            self.frame_index[i] += 1
            out[i] = {"init_x": init_x[sl], "pred_pose": pred[sl], "energy": energy[sl], "sorted_RTs": sorted_RTs[sl], "average_sRT": average_sRT[sl].clone(),
                      "nfev": smp.nlaunch - 1}
        return out


class DepthTracker:
    """Mask-free tracking of ONE sequence (ours; opt-in; the reference has no counterpart - its tracking loop cuts every frame's clouds out
    with the dataset's ground-truth masks, evaluation_tracking.py:262-337 - and no parity with it is claimed).  Around a
    FixedStepTracker(init='prior') that the caller constructs: after an object has been acquired once from a mask, its last pose and its
    size say where it is in the next depth frame, so a frame needs the depth image alone -
        acquire(depth, masks, rois, names)   clouds from the mask front end (DepthToClouds.device_clouds), one tracker step from the prior,
                                             then half = reward.cloud_extent(clouds, poses): the objects' sizes, fixed from here on;
        track(depth)                         clouds from depth and the stored boxes (DepthToClouds.device_clouds_boxes, draw run = the
                                             sequence's frame count), one tracker step, and the stored pose replaced only where the box
                                             gave a valid cloud: a LOST object keeps its previous pose, here and in the tracker's warm-start
                                             slot - a select on the device, in stream order.
    Both return the tracker's dict for the sequence plus points [n,n_pts,3], count [n] i32, valid [n] u8 (the front end's), half [n,3] and
    pose [n,4,4] (the stored poses after the select); between the depth upload and these device tensors nothing is read back.  The clouds
    of track() are the frame's native pixels inside the boxes, not the 256 x 256 crop-and-resize of the mask front end.  Sizes are not
    re-estimated, boxes do not reason about each other's occlusion, and a lost object is not re-acquired: call acquire again.
    trim: cloud_extent's (the trim + 1 largest |q_j| is the half-extent: 0 = the maximum); inflate, pad, min_count: device_clouds_boxes'."""

    def __init__(self, tracker, front_end=None, trim=0, inflate=1.15, pad=0.01, min_count=2):
        if getattr(tracker, "init", None) != "prior":
            raise ValueError("DepthTracker wraps a FixedStepTracker(init='prior'): it has no ground truth to start an object from")
        if int(trim) != trim or trim < 0:
            raise ValueError(f"DepthTracker(trim={trim}): an integer >= 0")
        if not (np.isfinite(inflate) and inflate > 0 and np.isfinite(pad) and pad >= 0):
            raise ValueError(f"DepthTracker(inflate={inflate}, pad={pad}): inflate finite > 0, pad finite >= 0")
        if int(min_count) != min_count or min_count < 0:
            raise ValueError(f"DepthTracker(min_count={min_count}): an integer >= 0")
        if front_end is None:
            from .preprocess import DepthToClouds
            front_end = DepthToClouds()
        self.tracker, self.fe = tracker, front_end
        self.trim, self.inflate, self.pad, self.min_count = int(trim), float(inflate), float(pad), int(min_count)
        self.names = self.rt = self.half = self.valid = None

    def acquire(self, depth, masks, rois, names, symmetric=None):
        """symmetric: None (the tracker's own `symmetric` callable, if it has one), a callable model_name -> bool or one flag per object -
        objects symmetric about their y axis measure one radius for x and z."""
        tr = self.tracker
        names = list(names)
        if not 1 <= len(names) <= tr.max_objects or len(names) != len(rois):
            raise ValueError(f"acquire: {len(names)} names for {len(rois)} rois; 1..max_objects_per_frame = {tr.max_objects} objects")
        if symmetric is None:
            symmetric = getattr(tr, "symmetric", None)
        sym = [bool(symmetric(nm)) for nm in names] if callable(symmetric) else symmetric
        tr.reset()
        fe = self.fe.device_clouds(depth, masks, rois, tr.seed, run=0)
        out = dict(tr.step([(fe["points"], names, None)])[0])
        half = reward.cloud_extent(fe["points"], out["average_sRT"], min(self.trim, fe["points"].shape[1] - 1), sym)
        self.names, self.rt, self.half, self.valid = names, out["average_sRT"].clone(), half, fe["valid"].clone()
        out.update(points=fe["points"], count=fe["count"], valid=fe["valid"], half=half, pose=self.rt)
        return out

    def track(self, depth):
        if self.names is None:
            raise RuntimeError("DepthTracker.track before acquire: there is no object to look for")
        tr = self.tracker
        n = len(self.names)
        fe = self.fe.device_clouds_boxes(depth, self.rt, self.half, tr.seed, run=tr.frame_index[0], inflate=self.inflate, pad=self.pad,
                                         min_count=self.min_count)
        out = dict(tr.step([(fe["points"], self.names, None)])[0])
        # a lost object keeps the pose it had: in this object's copy and in the slot the next frame's warm start reads
        self.rt = torch.where((fe["valid"] != 0).view(n, 1, 1), out["average_sRT"], self.rt)
        tr.pose_slots(0, n).copy_(self.rt)
        self.valid = fe["valid"]
        out.update(points=fe["points"], count=fe["count"], valid=fe["valid"], half=self.half, pose=self.rt)
        return out
