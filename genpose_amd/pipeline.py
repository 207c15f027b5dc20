"""Serving a stream of equally-shaped batches (throughput mode): request batching and stream pipelining around the agents'
kernels.  Three predictors, all returning per batch exactly what the sequential `PoseNet.pred_func` returns for it (asserted in
tests/test_gpu_pipeline.py):

  PipelinedPCPredictor  encoder + PC sampler.  `batches_per_launch` consecutive batches share one encoder pass and one sampler
                        launch chain (the sampler's batch-global coupling stays per batch, gp_pc_step_grouped); optionally the
                        encoder of the next group runs on a second HIP stream under the sampler graph of the current one
                        (`overlap`), and its furthest point sampling and ball queries always run ahead on a side stream (`fps_ahead`).
  GroupedODEPredictor   encoder + PF-ODE sampler, several batches per launch of the device-resident RK45 driver, one step
                        controller per batch (gp_rk45_phase_model).
  (runner.MultiSequenceTracker does the same for tracking, with ragged groups.)

Host code in these loops is allocation-free and keeps its CPU tensor ops single-threaded (see _randn_1t).
"""
import torch

from . import _lib
from .graphs import PinnedBlock
from .samplers import PCSampler
from .sde import SIGMA_MAX, SIGMA_MIN


def _randn_1t(out):
    """Standard-normal draw on the CPU generator into `out`, single-threaded: a multi-threaded CPU op leaves its OpenMP team
    spinning next to the HIP runtime's progress thread (see GFObjectPose._prior_to_device)."""
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        torch.randn(out.shape, out=out)
    finally:
        torch.set_num_threads(nt)


class PipelinedPCPredictor:
    """pred_func(encoder + PC sampler) for a stream of equally-shaped batches.

    score_agent : genpose_amd.posenet_agent.PoseNet (weights loaded, sampler_mode ['pc'])
    """

    def __init__(self, score_agent, B, K, num_steps, depth=2, sampler_streams=1, batches_per_launch=1, overlap=True, fps_ahead=True):
        """batches_per_launch = G > 1: G consecutive batches share every encoder and sampler launch (the batch-global
        coupling of the sampler stays per batch - gp_pc_step_grouped); at B*K = 3200 rows this lets the sampler run on
        32-row tiles (MFMA-bound) instead of 16-row tiles (weight-stream-bound): 21 vs 26 us per batch and step."""
        _lib.check_device()
        self.net = score_agent.net
        self.net.pointnet2_encoder(type(self).__name__)  # refuses an agent whose features are not the PointNet++ encoder's alone
        self.net._need_weights()
        self.G = batches_per_launch
        self.B1 = B                      # clouds per batch (the unit of the batch-global coupling)
        B = B * self.G                   # clouds per launch
        self.B, self.K, self.n, self.depth = B, K, num_steps, depth
        self.dev = self.net.device
        # the sampler is a latency-critical serial chain of short launches: its stream gets the HIGH hardware queue
        # priority so its workgroups are dispatched ahead of the encoder's thousands of queued workgroups
        self.s_enc = torch.cuda.Stream(self.dev, priority=0)
        # (sampler_streams > 1 puts several sampler chains in flight; measured SLOWER at the bench configuration:
        #  13.1 k vs 14.2 k poses/s - the chains contend for the same MFMA pipes and each step boundary gets longer)
        self.s_smp = [torch.cuda.Stream(self.dev, priority=-1) for _ in range(sampler_streams)] if overlap else [self.s_enc]
        # cfg.sampler_seed (opt-in): noise drawn inside the step kernels.  Batch i of the run() call number c draws as global rows
        # i * B*K .. with run index c - whatever launch it shares with other batches (PCSampler(seed=), run(row_base=))
        self.seed = getattr(self.net.cfg, "sampler_seed", None)
        self.runs = 0
        self.smp = [{self.G: PCSampler(self.net.pose_score_net, B, K, num_steps, self.dev, use_graph=True, record_traj=False, groups=self.G,
                                       precision=self.net._pc_precision(B, K, groups=self.G), seed=self.seed, products=self.net._pc_products())}
                    for _ in range(sampler_streams)]
        # furthest point sampling of the NEXT launch group runs on a side stream while the MFMA stages of the current group
        # own the chip: it is a latency-bound chain of 893 block-wide argmax steps per cloud (one workgroup per cloud, tiny
        # LDS), 7 % of the encoder when it runs alone, and fits next to the 8-wave sampler workgroups.
        self.fps_ahead = fps_ahead
        self.s_fps = torch.cuda.Stream(self.dev, priority=0) if fps_ahead else None
        self.ev_fps = [torch.cuda.Event() for _ in range(depth)]
        self.ev_enc_done = [torch.cuda.Event() for _ in range(depth)]  # encoder of a slot finished with its FPS workspace
        self.timing = False
        self.smp_events = []
        R = B * K
        self.cvec = [torch.empty(B, 768, device=self.dev) for _ in range(depth)]
        self.centre = [torch.empty(B, 3, device=self.dev) for _ in range(depth)]
        self.x0 = [torch.empty(R, 9, device=self.dev) for _ in range(depth)]
        self.ev_enc = [torch.cuda.Event() for _ in range(depth)]
        self.ev_free = [torch.cuda.Event() for _ in range(depth)]
        self.prior_host = [PinnedBlock((R, 9)) for _ in range(depth)]
        for e in self.ev_free:
            e.record(self.s_smp[0])

    def _sampler(self, j, g):
        if g not in self.smp[j]:  # ragged tail of a run: fewer batches in the last launch
            self.smp[j][g] = PCSampler(self.net.pose_score_net, self.B1 * g, self.K, self.n, self.dev, use_graph=True, record_traj=False, groups=g,
                                       precision=self.net._pc_precision(self.B1 * g, self.K, groups=g), seed=self.seed, products=self.net._pc_products())
        return self.smp[j][g]

    def run(self, batches, prior_noise=None, noise=None, out=None):
        """batches: sequence of device tensors [B,1024,3].  prior_noise: optional per-batch STANDARD-NORMAL draws [B*K,9]
        (scaled by sigma(1) here); noise: optional per-batch (z_langevin, z_predictor) draws (tests).
        Returns a list of pred_pose [B,K,9] float32 tensors (one per batch; written into `out[i]` when given)."""
        results = []
        run_index = self.runs
        self.runs += 1
        cur = torch.cuda.current_stream(self.dev)
        self.s_enc.wait_stream(cur)
        for st in self.s_smp:
            st.wait_stream(cur)
        B1, K, G = self.B1, self.K, self.G
        starts = list(range(0, len(batches), G))
        cat = lambda i0: batches[i0] if len(batches[i0:i0 + G]) == 1 else torch.cat(list(batches[i0:i0 + G]), dim=0)
        enc = self.net.pts_encoder
        staged = {}  # launch group -> concatenated clouds whose centres are being sampled on the side stream

        def stage_fps(c):
            if not self.fps_ahead or c >= len(starts):
                return
            slot = c % self.depth
            with torch.cuda.stream(self.s_fps):
                self.s_fps.wait_stream(cur)
                self.s_fps.wait_event(self.ev_enc_done[slot])  # the slot's previous centres are no longer read
                pts = cat(starts[c])
                pts.record_stream(self.s_enc)  # allocated here, consumed by the encoder stream
                # centres AND neighbourhoods: furthest point sampling is a latency-bound chain, the ball queries are LDS / VALU work -
                # neither touches the matrix pipes the sampler and the SA kernels are bound by
                ws = enc.prepare_grouping(pts, slot=slot)
                self.ev_fps[slot].record(self.s_fps)
            staged[c] = (pts, ws)

        for e in self.ev_enc_done:
            e.record(self.s_enc)
        stage_fps(0)
        for c, i0 in enumerate(starts):
            group = batches[i0:i0 + G]
            g = len(group)
            nb, nr = g * B1, g * B1 * K
            slot = c % self.depth
            # ---- encoder stage (stream E): features -> per-cloud embedding, prior -> device
            with torch.cuda.stream(self.s_enc):
                self.s_enc.wait_event(self.ev_free[slot])  # the sampler has consumed this slot's previous contents
                if c in staged:
                    pts, ws = staged.pop(c)
                    self.s_enc.wait_event(self.ev_fps[slot])
                    feat = enc.forward(pts, slot=slot, grouping=ws)
                else:
                    pts = cat(i0)
                    feat = enc.forward(pts, slot=slot)
                self.ev_enc_done[slot].record(self.s_enc)
            stage_fps(c + 1)  # queued behind nothing: runs under this group's remaining encoder stages and its sampler
            with torch.cuda.stream(self.s_enc):
                cv = self.net.pose_score_net.cloud_embed(feat)
                self.cvec[slot][:nb].copy_(cv)
                self.centre[slot][:nb].copy_(pts.mean(dim=1))
                x0 = self.x0[slot][:nr]
                if prior_noise is None:
                    # CPU generator, as sde.py:28.  (The slot's block waits for its previous copy: the host may run `depth` launches ahead,
                    # not further; the copy and its event go onto the current stream, s_enc)
                    self.prior_host[slot].send(self.x0[slot], lambda h: _randn_1t(h[:nr]), rows=nr)
                else:
                    x0.copy_(torch.cat([prior_noise[i0 + q].reshape(B1 * K, 9) for q in range(g)], dim=0))
                x0.mul_(SIGMA_MAX)  # prior std at T = 1 (cond_pc_sampler always starts from T = 1)
                self.ev_enc[slot].record(self.s_enc)
            # ---- sampler stage (stream S): the whole T-step loop as one graph replay
            j = c % len(self.s_smp)
            with torch.cuda.stream(self.s_smp[j]):
                self.s_smp[j].wait_event(self.ev_enc[slot])
                if noise is not None:
                    z1 = torch.cat([noise[i0 + q][0] for q in range(g)], dim=1)
                    z2 = torch.cat([noise[i0 + q][1] for q in range(g)], dim=1)
                else:
                    z1 = z2 = None
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) if self.timing else None
                seeded = {} if self.seed is None else dict(run_index=run_index, row_base=i0 * B1 * K)
                _, mean_x = self._sampler(j, g).run(self.cvec[slot][:nb], self.centre[slot][:nb], x0, z1, z2, slot_free_event=self.ev_free[slot],
                                                    graph_events=ev, **seeded)
                mean_x = mean_x.reshape(g, B1, K, 9)
                for q in range(g):
                    res = out[i0 + q] if out is not None else torch.empty(B1, K, 9, device=self.dev)
                    res.copy_(mean_x[q])
                    results.append(res)
                if ev is not None:
                    self.smp_events.append(ev + (g,))
        for st in self.s_smp:
            cur.wait_stream(st)
        cur.wait_stream(self.s_enc)
        if self.s_fps is not None:
            cur.wait_stream(self.s_fps)
        return results

    def sampler_launch_seconds(self):
        """Average duration of one pc_step launch inside the pipelined region (HIP events around every graph replay on
        the sampler streams; call after a synchronize)."""
        if not self.smp_events:
            return None
        tot = sum(a.elapsed_time(b) for a, b, _ in self.smp_events) * 1e-3
        return tot / (len(self.smp_events) * (self.n + 1))


class GroupedODEPredictor:
    """pred_func(encoder + PF-ODE sampler) for a stream of equally-shaped batches, `batches_per_launch` of them sharing every encoder
    pass and every launch of the device-resident RK45 driver.  Each batch keeps its own adaptive step control
    (gp_rk45_phase_model), i.e. gets what `PoseNet.pred_func` returns for it alone; the host only polls the per-batch status
    words between replays of the captured attempts."""

    def __init__(self, score_agent, B, K, T0=None, batches_per_launch=5):
        from .samplers import ODESampler
        _lib.check_device()
        self.net = score_agent.net
        self.net.pointnet2_encoder(type(self).__name__)  # refuses an agent whose features are not the PointNet++ encoder's alone
        self.net._need_weights()
        self.B1, self.K, self.G = B, K, batches_per_launch
        self.T0 = self.net.T if T0 is None else T0
        self.dev = self.net.device
        self._ODESampler = ODESampler
        self.trunk = getattr(self.net.cfg, "ode_trunk", None)  # opt-in: split-bf16 trunk where the launch runs the chain plan
        self.smp = {}
        self.last_nfev = []

    def _sampler(self, g):
        key = (g, self.trunk)
        if key not in self.smp:
            self.smp[key] = self._ODESampler(self.net.pose_score_net, self.B1 * g, self.K, self.dev, groups=g, trunk=self.trunk)
        return self.smp[key]

    def run(self, batches, prior_noise=None):
        """batches: sequence of device tensors [B,1024,3] -> list of pred_pose [B,K,9] float64 (one per batch).
        prior_noise (tests): per-batch STANDARD-NORMAL draws [B*K,9]; scaled by sigma(T0) here, exactly like the PC predictor
        scales its draws by sigma(1)."""
        self.last_nfev = []
        B1, K, G = self.B1, self.K, self.G
        n = len(batches)
        out = torch.empty(n, B1, K, 9, dtype=torch.float64, device=self.dev)  # one allocation per call, filled group by group
        if not hasattr(self, "_pts"):
            N = batches[0].shape[1]
            self._pts = torch.empty(G * B1, N, 3, device=self.dev)
            self._x0 = torch.empty(G * B1 * K, 9, device=self.dev)
            self._prior_host = PinnedBlock((G * B1 * K, 9))
        for i0 in range(0, n, G):
            g = min(G, n - i0)
            pts = self._pts[: g * B1]
            for q in range(g):
                pts[q * B1:(q + 1) * B1].copy_(batches[i0 + q])
            cvec = self.net.pose_score_net.cloud_embed(self.net.pts_encoder(pts))
            x0 = self._x0[: g * B1 * K]
            if prior_noise is None:
                # CPU generator, as sde.py:28; the block waits for the previous group's copy before the draw overwrites it
                self._prior_host.send(self._x0, lambda h: _randn_1t(h[: g * B1 * K]), rows=g * B1 * K)
            else:
                for q in range(g):
                    x0[q * B1 * K:(q + 1) * B1 * K].copy_(prior_noise[i0 + q].reshape(B1 * K, 9))
            x0.mul_(SIGMA_MIN * (SIGMA_MAX / SIGMA_MIN) ** self.T0)  # prior std at T0 (prior_noise = standard-normal draws, as in the PC predictor)
            smp = self._sampler(g)
            _, x = smp.run(cvec, pts.mean(dim=1), x0, self.T0, num_steps=self.net.cfg.sampling_steps, eps=self.net.sampling_eps)
            self.last_nfev += [int(s["nfev"]) for s in smp.group_stats]
            out[i0:i0 + g].copy_(x.reshape(g, B1, K, 9))
        return [out[i] for i in range(n)]


class FullPipelinePredictor:
    """BASELINE configs[2]: score model (encoder -> PC sampler) + energy model (encoder -> energy of every candidate) -> ranking ->
    top-`ratio` aggregation for one batch of B clouds - what `pred_func` -> `get_energy` -> `rank_aggregate` return when called one
    after the other (asserted in tests/test_gpu_fullsize.py), restructured around the one dependency that matters: the ENERGY
    encoder needs only the clouds, not the candidates.  It runs on a second HIP stream underneath the score model's sampler
    (whose step launches leave part of the chip idle: 12 800 rows = 400 32-row tiles = 1.56 rounds of the 256 CUs), and joins
    before the energy evaluation.

    score_agent / energy_agent : genpose_amd.posenet_agent.PoseNet with weights loaded (sampler_mode ['pc'] on the score agent)
    """

    def __init__(self, score_agent, energy_agent, B, K, num_steps, ratio=0.6, T_energy=1e-5, overlap=True, batches_per_launch=1, ranker="energy"):
        """batches_per_launch = G (run_many): G consecutive batches of B clouds share every encoder pass, the sampler launch chain
        (each batch keeps its own batch-global coupling, gp_pc_step_grouped), the energy evaluation and the ranking launch - the
        request batching of PipelinedPCPredictor applied to the whole pipeline.  At B = 256 one batch is 400 32-row tiles = 1.56 rounds
        of the CUs (the second round 56 % full); five batches are 2000 tiles = 7.8 rounds."""
        if ranker != "energy":
            raise NotImplementedError(f"FullPipelinePredictor(ranker={ranker!r}): this pipeline overlaps the ENERGY model's encoder with the sampler and "
                                      "ranks by its energies only; the likelihood ranker lives in SingleFrameRunner(ranker='likelihood')")
        _lib.check_device()
        self.snet, self.enet = score_agent.net, energy_agent.net
        for net in (self.snet, self.enet):
            net.pointnet2_encoder(type(self).__name__)  # refuses an agent whose features are not the PointNet++ encoder's alone
        self.snet._need_weights()
        self.enet._need_weights()
        if self.enet.cfg.posenet_mode != "energy" or self.snet.cfg.posenet_mode != "score":
            raise ValueError("FullPipelinePredictor(score_agent, energy_agent): agents in the wrong order / mode")
        self.B, self.K, self.n, self.ratio, self.G = B, K, num_steps, ratio, batches_per_launch
        self.dev = self.snet.device
        self.overlap = overlap
        self.share_grouping = self.snet.pts_encoder.grouping_key() == self.enet.pts_encoder.grouping_key()
        self.side = torch.cuda.Stream(self.dev, priority=0) if overlap else None
        self._smp = {}
        self.ev_side = torch.cuda.Event()
        R = self.G * B * K
        self.prior_host = PinnedBlock((R, 9))
        self.x0 = torch.empty(R, 9, device=self.dev)
        self.pose_e = torch.empty(R, 9, device=self.dev)
        t = torch.full((1,), float(T_energy), device=self.dev)
        self.tvec_e = self.enet.pose_score_net.time_embed(t)[0].contiguous()
        self.sigma_e = (SIGMA_MIN * (SIGMA_MAX / SIGMA_MIN) ** t).contiguous()

    def _sampler(self, g):
        if g not in self._smp:
            # cfg.sampler_seed of the score agent (opt-in): noise drawn inside the step kernels; batch i of call number c draws as global
            # rows i * B*K .. with run index c, whatever launch it shares (as PipelinedPCPredictor)
            self._smp[g] = PCSampler(self.snet.pose_score_net, g * self.B, self.K, self.n, self.dev, use_graph=True, record_traj=False, groups=g,
                                     seed=getattr(self.snet.cfg, "sampler_seed", None), products=self.snet._pc_products())
        return self._smp[g]

    def run(self, pts, prior_noise=None, noise=None):
        """pts [B,1024,3] device tensor -> dict(pred_pose [B,K,9] f32, energy [B,K,2], sorted_poses, sorted_energy, order, avg_pose [B,7]).
        prior_noise (tests): standard-normal draws [B*K,9]; noise (tests): (z_langevin, z_predictor) [n,B*K,9]."""
        if pts.shape[0] != self.B:
            raise ValueError(f"predictor built for {self.B} clouds got {pts.shape[0]}")
        self._runs = getattr(self, "_runs", 0) + 1
        return self._run_group(pts, 1, prior_noise, noise, self._runs - 1, 0)

    def run_many(self, batches, prior_noise=None, noise=None):
        """batches: sequence of device tensors [B,1024,3] -> one result dict per batch (views into the launch group's tensors);
        `batches_per_launch` of them share every launch.  prior_noise / noise (tests): per-batch draws as in run()."""
        out = []
        self._runs = getattr(self, "_runs", 0) + 1
        for i0 in range(0, len(batches), self.G):
            grp = list(batches[i0:i0 + self.G])
            g = len(grp)
            pts = grp[0] if g == 1 else torch.cat(grp, dim=0)
            pn = None if prior_noise is None else torch.cat([prior_noise[i0 + q].reshape(self.B * self.K, 9) for q in range(g)], dim=0)
            nz = None if noise is None else (torch.cat([noise[i0 + q][0] for q in range(g)], dim=1), torch.cat([noise[i0 + q][1] for q in range(g)], dim=1))
            res = self._run_group(pts, g, pn, nz, self._runs - 1, i0 * self.B * self.K)
            for q in range(g):
                sl = slice(q * self.B, (q + 1) * self.B)
                out.append({k: (v[sl] if v is not None else None) for k, v in res.items()})
        return out

    def _run_group(self, pts, g, prior_noise, noise, run_index=0, row_base=0):
        from . import reward
        B, K = g * self.B, self.K
        cur = torch.cuda.current_stream(self.dev)
        centre = pts.mean(dim=1)
        # ---- centres and neighbourhoods (furthest point sampling, ball queries) depend on the coordinates only: computed ONCE and
        # used by both encoders (the reference computes them twice, once per agent)
        enc_s, enc_e = self.snet.pts_encoder, self.enet.pts_encoder
        grouping = enc_s.prepare_grouping(pts) if self.share_grouping else None
        # ---- energy model's encoder + per-cloud embedding: depends on the clouds only -> side stream
        if self.side is not None:
            self.side.wait_stream(cur)
            with torch.cuda.stream(self.side):
                cvec_e = self.enet.pose_score_net.cloud_embed(enc_e.forward(pts, grouping=grouping))
                self.ev_side.record(self.side)
            cvec_e.record_stream(cur)
        # ---- score model: encoder -> embedding -> prior -> the whole T-step loop as one graph replay
        cvec = self.snet.pose_score_net.cloud_embed(enc_s.forward(pts, grouping=grouping))
        x0 = self.x0[: B * K]
        if prior_noise is None:
            self.prior_host.send(self.x0, lambda h: _randn_1t(h[: B * K]), rows=B * K)  # CPU generator, as sde.py:28; the copy goes onto `cur`
        else:
            x0.copy_(prior_noise.reshape(B * K, 9))
        x0.mul_(SIGMA_MAX)
        z1, z2 = noise if noise is not None else (None, None)
        smp = self._sampler(g)
        seeded = {} if smp.seed is None else dict(run_index=run_index, row_base=row_base)
        _, mean_x = smp.run(cvec, centre, x0, z1, z2, **seeded)
        pred = mean_x.reshape(B, K, 9).clone()
        # ---- energy of every candidate (posenet_agent.py:471-527: translations relative to the cloud centre), ranking, aggregation
        if self.side is not None:
            cur.wait_event(self.ev_side)
        else:
            cvec_e = self.enet.pose_score_net.cloud_embed(enc_e.forward(pts, grouping=grouping))
        pose_flat = self.pose_e[: B * K]
        pose = pose_flat.view(B, K, 9)
        pose.copy_(pred)
        pose[:, :, 6:] -= centre.unsqueeze(1)
        energy = self.enet.pose_score_net.evaluate(cvec_e, K, pose_flat, self.tvec_e, self.sigma_e, "energy").reshape(B, K, 2)
        out = reward.rank_aggregate(pred, energy, ratio=self.ratio)
        out["pred_pose"], out["energy"] = pred, energy
        return out
