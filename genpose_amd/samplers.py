"""Samplers on the HIP kernels: cond_pc_sampler / cond_ode_sampler of networks/gf_algorithms/samplers.py:102-227
(pose_mode 'rot_matrix', VE SDE), and cond_edm_sampler's fixed-step Heun method (:230-290) on the same probability-flow ODE.  Host code only builds schedule tables, owns buffers and replays hipGraphs;
every per-step operation runs in csrc/scorenet.hip / csrc/rk45.hip.
"""
import numpy as np
import torch

from . import _lib
from ._lib import ptr, stream_ptr
from .graphs import PinnedBlock, capture
from .sde import EPS, SIGMA_MAX, SIGMA_MIN, ve_sde


def pc_schedule(num_steps, eps=EPS):
    """Host schedule table of the PC sampler: [num_steps,4] = sigma(t_i), g(t_i), step_size, sqrt(step_size),
    evaluated with the reference's own f32 tensor expressions (samplers.py:118-119,145; sde.py:15-24)."""
    time_steps = torch.linspace(1.0, eps, num_steps)
    step_size = time_steps[0] - time_steps[1]
    bt = time_steps.reshape(-1, 1)
    sigma = SIGMA_MIN * (SIGMA_MAX / SIGMA_MIN) ** bt
    _, g = ve_sde(bt)
    sched = torch.cat([sigma, g, step_size.expand(num_steps, 1), torch.sqrt(step_size).expand(num_steps, 1)], dim=1)
    return time_steps, sched.float().contiguous()


class PCSampler:
    """Predictor-corrector sampler state for a fixed (B, K, num_steps): buffers + optional hipGraph of the whole loop."""

    def __init__(self, net, B, K, num_steps, device, use_graph=True, record_traj=False, groups=1, coupling_group=None, tile=0, model="score",
                 precision="f32", trunk=None, seed=None, row_base=None, products=None):
        """B clouds in `groups` independent batches of B/groups clouds laid out back to back: one launch chain serves all of
        them, the batch-mean gradient norm (samplers.py:130-132) stays per batch (gp_pc_step_grouped).

        coupling_group (a torch.distributed process group; "faithful" multi-GPU mode, SURVEY §8e caveat): this rank's B clouds are
        one SHARD of a batch that is spread over the ranks of the group (equal shards).  After every step the per-batch sums of
        |score| are all-reduced (one float per batch) and the next launch takes the mean over ALL rows of the batch
        (gp_pc_step_plan with gn_ext), so every shard steps exactly as the unsharded batch would.  On RCCL (backend 'nccl') the
        per-step reduction - one device-side sum and one all-reduce of `groups` floats - is captured INSIDE the sampler's hipGraph
        with the launches; on gloo (CPU tests, two ranks sharing one device) the loop runs launch by launch."""
        if B % groups:
            raise ValueError(f"{B} clouds do not split into {groups} equal batches")
        if model not in ("score", "energy"):
            raise ValueError(model)
        # seed (OPT-IN; an integer, taken modulo 2^64): the noise of both streams is drawn inside the step kernels by a counter-based
        # generator (csrc/philox.h: Philox4x32-10 + Box-Muller keyed by seed, run index, step, stream and GLOBAL row = row_base + row of
        # the launch) instead of torch's device generator: no z1 / z2 buffers, and a row draws the same values under every launch plan,
        # in any batch of a launch (the caller gives the launch the base of its first row) and on any shard.  The seed state lives in a
        # small device buffer the captured launches read: one pinned-memory copy in stream order before each replay updates it.
        # seed=None: nothing changes.
        if seed is not None:
            if precision == "bf16x3":
                raise NotImplementedError("seed= with precision='bf16x3': the split-bf16x3 PC step has no seeded kernel")
            if model == "energy":
                raise NotImplementedError("seed= with model='energy': the energy model's PC step has no seeded kernel")
            if coupling_group is not None and groups > 1:
                raise NotImplementedError("seed= with coupling_group and groups > 1: one row base cannot place the shards of several batches")
        elif row_base is not None:
            raise ValueError("row_base= needs seed=")
        # precision 'bf16x3' (OPT-IN, exploratory; csrc/trunk_bf16x3.hip): the trunk's dense layers as three-term bf16 split products with
        # fp32 accumulation, 128-row workgroups.  Score model, no cross-rank coupling; never the default.
        if precision not in ("f32", "bf16x3"):
            raise ValueError(f"sampler precision {precision!r}: 'f32' or 'bf16x3'")
        if precision == "bf16x3" and (model != "score" or coupling_group is not None or tile):
            raise NotImplementedError("the split-bf16 PC step serves the score model, uncoupled, on its own launch plan")
        self.precision = precision
        # model 'energy': `net` holds the ENERGY network's weights and the sampler is driven by ITS score - the gradient of the
        # inner-product energy (posenet.py:94-130 on a PoseEnergyNet), evaluated inside the step kernel (forward + vector-Jacobian product)
        self.model = 0 if model == "score" else 1
        self.net, self.B, self.K, self.n, self.groups = net, B, K, num_steps, groups
        self.dev = torch.device(device)
        R = B * K
        self.R = R
        # launch plan (csrc/score_trunk.h: score_plan_rows): 16 / 32 / 64 = tile form, 128 = chain form (register-resident trunk, weights
        # through an LDS ring) for launches of ~32 000 rows and more; `tile` forces one (tests, measurements)
        import ctypes
        t_out, n_out = ctypes.c_int(0), ctypes.c_int(0)
        if precision == "bf16x3":
            if _lib.lib().gp_pc_layout_bf16x3(groups, B // groups, K, ctypes.byref(n_out)) != 0:
                raise ValueError(f"{B // groups} clouds x {K} candidates per batch do not split into 128-row workgroups of at most four clouds")
            t_out.value = 128
            self._bf = net.w.bf16x3_packs()
        elif _lib.lib().gp_pc_layout(self.model, int(tile), groups, B // groups, K, ctypes.byref(t_out), ctypes.byref(n_out)) != 0:
            raise ValueError(f"{B // groups} clouds x {K} candidates per batch do not split into workgroups of plan {tile or 'auto'}; "
                             "run the batches separately")
        if coupling_group is not None and (t_out.value & _lib.PLAN_HEADSPLIT):
            # a sharded batch: the per-step sums below run over whole-tile partials - the plain 16-row tiles, not the head-split plan
            if _lib.lib().gp_pc_layout(self.model, 16, groups, B // groups, K, ctypes.byref(t_out), ctypes.byref(n_out)) != 0:
                raise ValueError("16-row tiles do not fit this batch")
        # self.plan is what the launches are given; self.tile the rows per workgroup of it; self.hsplit = 3 under the head-split plan of
        # the latency regime (three workgroups per 16-row tile, one head of the network each - GP_PLAN_HEADSPLIT)
        self.plan, self.nparts = t_out.value, n_out.value
        self.tile, self.hsplit = self.plan & ~_lib.PLAN_HEADSPLIT, (3 if self.plan & _lib.PLAN_HEADSPLIT else 1)
        # trunk: the arithmetic of the score model's chain plan (128 rows per workgroup) - 'bf16x9' (the default: csrc/trunk_bf16x9.hip,
        # every fp32 product as the nine exact products of hi / mid / lo bf16 terms on the BF16 matrix pipe, fp32 accumulation) or
        # 'f32mfma' (pc_step_chain_kernel<2>: fp32 MFMA; A/B runs and tests).  Every other plan, model and precision ignores it.
        if trunk not in (None, "bf16x9", "f32mfma"):
            raise ValueError(f"trunk {trunk!r}: 'bf16x9' or 'f32mfma'")
        # products: how many of the nine cross products the bf16x9 trunk issues - None / 9 (the class default: all nine, the kernels whose
        # bits are recorded) or 6 (lo.lo, lo.mid and mid.lo are not issued, csrc/bf16x9.h: at most (2^-23 + 2^-32) |a b| per multiply, below
        # the fp32 accumulation's own rounding; gp_pc_step_bf16x6 and its seeded twin).  Read only where trunk == 'bf16x9' applies; every
        # other plan, model, precision and trunk ignores it, as they ignore `trunk` (self.products is then None).
        if products not in (None, 9, 6):
            raise ValueError(f"products {products!r}: 9 or 6")
        self.trunk = None
        if precision == "f32" and self.model == 0 and self.tile == 128:
            self.trunk = trunk or "bf16x9"
            if self.trunk == "bf16x9":
                self._x9 = net.w.bf16x9_packs()
        self.products = (products or 9) if self.trunk == "bf16x9" else None
        self._x9_entry = "gp_pc_step_bf16x6" if self.products == 6 else "gp_pc_step_bf16x9"
        if precision == "bf16x3":
            self.kernel_name = "pc_step_bf16x3_kernel"
        elif self.trunk == "bf16x9":
            self.kernel_name = "pc_step_chain_kernel<bf16x9,6>" if self.products == 6 else "pc_step_chain_kernel<bf16x9>"
        elif self.tile in (16, 32, 64):
            self.kernel_name = ("pc_step_kernel<16,0,split>" if self.hsplit == 3 else f"pc_step_kernel<{self.tile}>" if self.model == 0
                                else f"pc_step_kernel<{self.tile},energy>")
        else:
            self.kernel_name = "pc_step_chain_kernel<2>" if self.model == 0 else "pc_step_chain_kernel<2,energy>"
        ts, sched = pc_schedule(num_steps)
        self.sched = sched.to(self.dev)
        self.tvec_all = net.time_embed(ts.to(self.dev))
        f = lambda *s: torch.empty(*s, device=self.dev)
        self.x, self.mean_x, self.score = f(R, 9), f(R, 9), f(R, 9)
        self.partials = torch.zeros(num_steps, self.nparts, device=self.dev)
        self.seed = None if seed is None else int(seed) % (1 << 64)
        if self.seed is None:
            self.z1, self.z2 = f(num_steps, R, 9), f(num_steps, R, 9)
        else:
            self.z1 = self.z2 = None
            self.seed_state = torch.zeros(4, dtype=torch.int64, device=self.dev)  # gp_philox::SEED_WORDS uint32: seed, run index, row base, 0
            self._seed_host = PinnedBlock(4, torch.int64)
            self.next_run_index = 0
            self.last_run_index = None
        self.cvec, self.centre = f(B, 768), f(B, 3)
        self.traj = f(num_steps, R, 9) if record_traj else None
        self.coupling_group = coupling_group
        self.gn_ext, self.gn_rows = None, 0
        if coupling_group is not None:
            import torch.distributed as dist
            self._dist = dist
            self._world = dist.get_world_size(coupling_group)
            self.gn_ext = torch.zeros(num_steps, groups, device=self.dev)
            self.gn_rows = R // groups * self._world  # rows of a batch over all its (equal) shards
            use_graph = use_graph and dist.get_backend(coupling_group) == "nccl"  # an RCCL all-reduce is graph-capturable, a gloo one is not
        self.use_graph = use_graph
        self.graph = None
        self.captures = 0
        if self.seed is not None:
            # a shard of a batch draws the rows it holds of the unsharded batch
            rank = self._dist.get_rank(coupling_group) if coupling_group is not None else 0
            self.row_base = int(row_base) if row_base is not None else rank * R

    def reseed(self, seed):
        """A new seed for the following runs (the run index starts again at 0); captured launches follow it."""
        if self.seed is None:
            raise ValueError("reseed() on a sampler built without seed=")
        self.seed = int(seed) % (1 << 64)
        self.next_run_index = 0

    def _write_seed_state(self, run_index, row_base):
        if run_index is None:
            run_index = self.next_run_index
            self.next_run_index = (run_index + 1) % (1 << 32)
        words = _lib.seed_words(self.seed, run_index, self.row_base if row_base is None else row_base)  # (ValueError: run or base out of range)
        self.last_run_index = int(run_index)
        self._seed_host.send(self.seed_state, lambda h: h.copy_(torch.from_numpy(words.view(np.int64))))

    def launch_step(self, i):
        """Launch i of the chain (0 <= i <= n) on the current stream: finishes step i-1 and, for i < n, evaluates the score at t_i."""
        shape = (self.groups, self.B // self.groups, self.K, i, self.n)
        gn = (ptr(self.gn_ext), self.gn_rows)
        if self.seed is not None:
            bufs = (ptr(self.cvec), ptr(self.tvec_all), ptr(self.sched), ptr(self.seed_state), ptr(self.centre), ptr(self.x), ptr(self.mean_x),
                    ptr(self.score), ptr(self.partials), ptr(self.traj))
            if self.trunk == "bf16x9":
                _lib.call(self._x9_entry + "_seeded", *shape, self.net.w.ref(), *bufs, *gn, *(ptr(w) for w in self._x9), stream_ptr())
            else:
                _lib.call("gp_pc_step_plan_seeded", self.plan, *shape, self.net.w.ref(), *bufs, *gn, stream_ptr())
            return
        bufs = (ptr(self.cvec), ptr(self.tvec_all), ptr(self.sched), ptr(self.z1), ptr(self.z2), ptr(self.centre), ptr(self.x), ptr(self.mean_x),
                ptr(self.score), ptr(self.partials), ptr(self.traj))
        if self.precision == "bf16x3":
            t = self.net.w.tensors
            _lib.call("gp_pc_step_bf16x3", *shape, *bufs, *(ptr(w) for w in self._bf), ptr(t["b_pose0"]), ptr(t["b_pose2"]), ptr(t["w_out"]),
                      ptr(t["b_out"]), stream_ptr())
        elif self.trunk == "bf16x9":
            _lib.call(self._x9_entry, *shape, self.net.w.ref(), *bufs, *gn, *(ptr(w) for w in self._x9), stream_ptr())
        else:
            _lib.call("gp_pc_step_plan", self.model, self.plan, *shape, self.net.w.ref(), *bufs, *gn, stream_ptr())

    def _launch_all(self):
        for i in range(self.n + 1):
            self.launch_step(i)
            if self.coupling_group is not None and i < self.n:
                # sum of |score_i| over this shard's rows, per batch -> over all shards (the kernel divides by the batch's row count)
                torch.sum(self.partials[i].view(self.groups, -1), dim=1, out=self.gn_ext[i])
                self._dist.all_reduce(self.gn_ext[i], op=self._dist.ReduceOp.SUM, group=self.coupling_group)

    def run(self, cvec, centre, init_x, z_langevin=None, z_predictor=None, slot_free_event=None, graph_events=None, run_index=None, row_base=None):
        """cvec [B,768], centre [B,3], init_x [R,9]; noise [n,R,9] (drawn on the device generator if None).
        Returns (xs [R,n,9] or None, mean_x [R,9]) float32, like cond_pc_sampler.
        slot_free_event: recorded once the inputs have been copied into the sampler's own buffers (pipelining).
        A seeded sampler (seed=) draws its own noise: every run() takes the next run index (other draws), run_index= pins it (a
        repeated index repeats the draws), row_base= places this launch's first row (default: the constructor's)."""
        if self.seed is None and (run_index is not None or row_base is not None):
            raise ValueError("run_index= / row_base= need a sampler built with seed=")
        if self.seed is not None and (z_langevin is not None or z_predictor is not None):
            raise ValueError("explicit z_langevin= / z_predictor= on a seeded sampler: it draws its own noise (build it without seed= to inject noise)")
        self.cvec.copy_(cvec)
        self.centre.copy_(centre)
        self.x.copy_(init_x)
        if slot_free_event is not None:
            slot_free_event.record(torch.cuda.current_stream())
        if self.seed is not None:
            self._write_seed_state(run_index, row_base)
        elif z_langevin is None:
            self.z1.normal_()
            self.z2.normal_()
        else:
            self.z1.copy_(z_langevin)
            self.z2.copy_(z_predictor)
        if not self.use_graph:
            self._launch_all()
        else:
            _replay_captured(self, self.x.clone() if self.graph is None else None, graph_events)
        xs = self.traj.permute(1, 0, 2) if self.traj is not None else None
        return xs, self.mean_x


def _replay_captured(smp, restore, graph_events=None):
    """The graph path of a sampler's run().  First run: a warm-up chain outside capture (it sets the kernels' attributes), smp.x put back
    from `restore`, the whole chain captured once.  Every run: the replay, between graph_events' two events where given."""
    if smp.graph is None:
        # (no `bufs`: run() has filled the sampler's own buffers, which the launch-by-launch path reads as well)
        smp._captured = capture(smp._launch_all, warmup=lambda: (smp._launch_all(), smp.x.copy_(restore)))
        smp.graph = smp._captured.graph
        smp.captures += 1
    smp._captured.replay(events=graph_events)


class _ScheduleTable:
    """A fixed-step solver's run-time schedule: [launches][row] floats + the N + 1 times, one pinned block -> one device block (sched,
    t_dev) -> the time-embedding table (tvec_all), refilled in stream order when the key changes.  classes = C > 1 (schedule classes): C
    schedules [C][launches][row] and C x (N + 1) times in the same one block, one gp_time_embed over all of them -> tvec_all [C (N+1), 768]."""

    def __init__(self, net, nlaunch, row, ntimes, device, classes=1):
        self.net, self.dev = net, device
        self._sched_len = classes * nlaunch * row
        ntimes = classes * ntimes
        self._table = torch.zeros(self._sched_len + ntimes, device=device)
        self._host = PinnedBlock(self._sched_len + ntimes)
        self._key = None
        self.sched = self._table[: self._sched_len]
        self.t_dev = self._table[self._sched_len:]
        self.tvec_all = torch.empty(ntimes, 768, device=device)

    def write(self, key, schedule):
        """schedule() -> (times [N + 1], sched [launches][row]) - with classes, both stacked over the classes; called only when `key` is not
        the one the buffers hold."""
        if key == self._key:
            return
        t, sched = schedule()

        def fill(host):
            h = host.numpy()
            h[: self._sched_len] = sched.reshape(-1)
            h[self._sched_len:] = t.astype(np.float32).reshape(-1)
        self._host.send(self._table, fill)
        self.net.time_embed(self.t_dev, out=self.tvec_all)
        self._key = key


def pc_noise_fill(seed, run_index, num_steps, nrows, device, row_base=0, step0=0, row0=0):
    """The draws of a seeded PC sampler as buffers (gp_pc_noise_fill: the step kernels' own device function): (z_langevin, z_predictor),
    [num_steps, nrows, 9] each, for steps step0 .. and rows row0 .. of a launch whose first row is global row `row_base`.  Feeding them to
    an unseeded sampler's run(z_langevin=, z_predictor=) reproduces the seeded run bit for bit."""
    dev = torch.device(device)
    st = _seed_state(seed, run_index, row_base, dev)
    z1, z2 = torch.empty(num_steps, nrows, 9, device=dev), torch.empty(num_steps, nrows, 9, device=dev)
    _lib.call("gp_pc_noise_fill", ptr(st), int(step0), int(num_steps), int(row0), int(nrows), ptr(z1), ptr(z2), stream_ptr())
    return z1, z2


def _seed_state(seed, run_index, row_base, device):
    """_lib.seed_words as the int64 [4] tensor the seeded entry points take, on `device`."""
    return torch.from_numpy(_lib.seed_words(seed, run_index, row_base).view(np.int64)).to(device)


def track_prior_fill(seed, frame_index, nrows, device, row_base=0, row0=0):
    """The fixed-step tracker's prior draws as a buffer (gp_track_prior_fill: track_warm_start's own device function): standard normals
    [nrows, 9] for rows row0 .. of a launch whose first row is global row `row_base`, frame `frame_index` (the seed state's run word)."""
    dev = torch.device(device)
    st = _seed_state(seed, frame_index, row_base, dev)
    z = torch.empty(nrows, 9, device=dev)
    _lib.call("gp_track_prior_fill", ptr(st), int(row0), int(nrows), ptr(z), stream_ptr())
    return z


def track_warm_start(seed_state, sigma, prev_sRT, src, fallback_sRT, centre, K, out=None):
    """The tracker's start states on the device (gp_track_warm_start; evaluation_tracking.py:302-310 + samplers.py:180): for cloud i and
    candidate k, x0[i K + k] = init_i + sigma z with init_i = [R[:,0], R[:,1], t - centre[i]] of prev_sRT[src[i]] (src[i] >= 0) or of
    fallback_sRT[i], z the prior's draw for global row (row base + i K + k) of the seed state's frame.  seed_state: 8 uint32 words on the
    device (csrc/philox.h); sigma: a one-element device tensor; prev_sRT, fallback_sRT [.,4,4] f32; src [n] int32; centre [n,3]."""
    n = int(centre.shape[0])
    for t, dt in ((sigma, torch.float32), (prev_sRT, torch.float32), (fallback_sRT, torch.float32), (centre, torch.float32), (src, torch.int32)):
        if t.dtype != dt:
            raise ValueError(f"track_warm_start: expected {dt}, got {t.dtype}")
    if src.shape[0] != n or fallback_sRT.shape[0] != n:
        raise ValueError(f"track_warm_start: {n} clouds, src {tuple(src.shape)}, fallback_sRT {tuple(fallback_sRT.shape)}")
    if out is None:
        out = torch.empty(n * int(K), 9, device=centre.device)
    _lib.call("gp_track_warm_start", n, int(K), ptr(seed_state), ptr(sigma), ptr(prev_sRT), ptr(src), ptr(fallback_sRT), ptr(centre), ptr(out), stream_ptr())
    return out


def track_start_classes(seed_state, sched, class_stride, prev_sRT, src, fallback_sRT, centre, K, acquire=True, out=None, cls_out=None):
    """The tracker's start states with a schedule class per cloud (gp_track_start_classes): track_warm_start that can ACQUIRE.  sched: a
    class-aware sampler's schedule block (HeunSampler(classes=C).sched), class_stride = launches * floats per row.  Cloud i with src[i] >= 0
    gets track_warm_start's bits on class 0's sigma; with src[i] < 0 and acquire, the pure prior sigma_1 z on the same draw (samplers.py:180
    with init_x = None; fallback_sRT may be None), without acquire the fallback pose.  Returns (x0 [n K, 9], cls [n] int32: the class table of
    the solve, made on the device)."""
    n = int(centre.shape[0])
    for t, dt in ((sched, torch.float32), (prev_sRT, torch.float32), (centre, torch.float32), (src, torch.int32)) + (() if fallback_sRT is None else ((fallback_sRT, torch.float32),)):
        if t.dtype != dt:
            raise ValueError(f"track_start_classes: expected {dt}, got {t.dtype}")
    if fallback_sRT is None and not acquire:
        raise ValueError("track_start_classes: fallback_sRT=None needs acquire=True")
    if src.shape[0] != n or (fallback_sRT is not None and fallback_sRT.shape[0] != n):
        raise ValueError(f"track_start_classes: {n} clouds, src {tuple(src.shape)}, fallback_sRT {None if fallback_sRT is None else tuple(fallback_sRT.shape)}")
    if acquire and sched.numel() <= int(class_stride):
        raise ValueError("track_start_classes: acquire reads class 1's sigma, the schedule block holds one class")
    if out is None:
        out = torch.empty(n * int(K), 9, device=centre.device)
    if cls_out is None:
        cls_out = torch.empty(n, dtype=torch.int32, device=centre.device)
    _lib.call("gp_track_start_classes", n, int(K), ptr(seed_state), ptr(sched), int(class_stride), ptr(prev_sRT), ptr(src), ptr(fallback_sRT), ptr(centre),
              ptr(out), ptr(cls_out), int(bool(acquire)), stream_ptr())
    return out, cls_out


def philox_raw(counters, keys):
    """Raw Philox4x32-10 blocks on the device: counters [n,4], keys [n,2] (int32 tensors holding the uint32 words) -> [n,4]."""
    counters, keys = counters.contiguous(), keys.contiguous()
    out = torch.empty_like(counters)
    _lib.call("gp_philox_raw", counters.shape[0], ptr(counters), ptr(keys), ptr(out), stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------- PF-ODE (fixed-step Heun)
HEUN_GRIDS = ("geometric", "edm")
_HEUN_G_FACTOR = np.float32(4.1272735595703125)  # (float)sqrt(2 (ln 50 - ln 0.01)): g(t) = sigma(t) * this, in f32 like the RK45 driver's denoise


def heun_launches(nsteps, denoise=True):
    """Launches of a Heun chain (gp_heun_launches): 2 N + 1, one more with denoise.  NFE = launches - 1."""
    if int(nsteps) < 1:
        raise ValueError(f"nsteps {nsteps}: at least one step")
    return 2 * int(nsteps) + 1 + (1 if denoise else 0)


def heun_grid(nsteps, T0=1.0, eps=EPS, grid="geometric", rho=7.0):
    """Times t_0 = T0 > ... > t_N = eps and their sigma_i = sigma_min (sigma_max / sigma_min)^t_i, float64.
    'geometric': t uniform from T0 to eps (sigma geometric); 'edm': cond_edm_sampler's rho discretisation (samplers.py:241-242) between
    sigma(T0) and sigma(eps), mapped back to t.  Both end exactly at eps."""
    N = int(nsteps)
    if N < 1:
        raise ValueError(f"nsteps {nsteps}: at least one step")
    if grid not in HEUN_GRIDS:
        raise ValueError(f"heun grid {grid!r}: one of {HEUN_GRIDS}")
    if not 0.0 < eps < T0:
        raise ValueError(f"need 0 < eps < T0, got eps {eps}, T0 {T0}")
    ratio = SIGMA_MAX / SIGMA_MIN
    if grid == "geometric":
        t = np.linspace(float(T0), float(eps), N + 1)
    else:
        s_hi, s_lo = SIGMA_MIN * ratio ** float(T0), SIGMA_MIN * ratio ** float(eps)
        idx = np.arange(N + 1, dtype=np.float64)
        s = (s_hi ** (1.0 / rho) + idx / N * (s_lo ** (1.0 / rho) - s_hi ** (1.0 / rho))) ** rho
        t = np.log(s / SIGMA_MIN) / np.log(ratio)
    t[0], t[-1] = float(T0), float(eps)
    return t, SIGMA_MIN * ratio ** t


def heun_schedule(nsteps, T0=1.0, eps=EPS, grid="geometric", rho=7.0, denoise=True):
    """Host schedule of a Heun chain: (t [N+1] f64, sched [launches,4] f32) - per launch the sigma of its evaluation (the score's divisor),
    the slope factor, the step h and the launch kind (include/genpose_hip.h: gp_heun_step_plan), computed in float64 and rounded once."""
    N = int(nsteps)
    t, sig = heun_grid(N, T0, eps, grid, rho)
    h = sig[1:] - sig[:-1]
    sched = np.zeros((heun_launches(N, denoise), 4), dtype=np.float64)
    sched[0] = (sig[0], 0.0, 0.0, 0.0)
    for i in range(N):
        sched[2 * i + 1] = (sig[i + 1], -sig[i], h[i], 1.0)
        sched[2 * i + 2] = (sig[i + 1], -sig[i + 1], h[i], 2.0)
    if denoise:
        # the reverse-diffusion predictor at eps (samplers.py:209-218) with cond_ode_sampler's divisor rule for num_steps = N
        g = np.float32(sig[N]) * _HEUN_G_FACTOR
        sched[2 * N + 1] = (sig[N], g, (1.0 - float(eps)) / N, 4.0)
    else:
        sched[2 * N, 3] = 3.0
    return t, sched.astype(np.float32)


class HeunSampler:
    """Fixed-step Heun solver of the probability-flow ODE, integrated in sigma: cond_edm_sampler's second-order method
    (samplers.py:230-290) driven by the VE score model (slope d = -sigma score), state in fp32.  Deterministic, fixed NFE = 2 N (+ 1 with
    denoise), row-local: one captured launch chain per geometry, nothing read back, the same latency on every frame; N trades accuracy for
    time.  T0 and eps are run-time values: the schedule and the time-embedding table are device buffers refilled in stream order before a
    replay, so a tracker that changes T0 per frame never recaptures.

    B clouds in `groups` batches laid out back to back share each launch (a workgroup never straddles two of them); the result of a row
    does not depend on its neighbours.  trunk: as PCSampler - 'bf16x9' on the chain plan by default, 'f32mfma' for A/B.  tile: forces a
    plan (16 / 32 / 64 tiles, 128 chain form); the head-split plan and bf16x3 have no Heun kernel.

    model: 'score' (default) | 'energy' (ours; opt-in) - `net` holds the ENERGY network's weights and ITS score, the gradient of the
    inner-product energy (energynet.py:200-222), drives the solver: forward + vector-Jacobian product inside the kernels (the `_model` entry
    points), plans 16 and 128 only (gp_heun_layout_model), fp32 MFMA only (trunk None / 'f32mfma'), launches='single' on plan 16.
    Schedules, grids, buffers, run-time T0 / eps, graph capture and last_stats are the score model's.

    launches: 'chain' (default) - one kernel launch per launch index; 'single' - the whole solve in ONE launch (gp_heun_solve_tile: a
    workgroup takes its tile's rows through every index itself, tile plans only), the same bits in x, the pose and the trajectory.  nlaunch,
    NFE and the schedule are those of the chain either way.

    classes: C > 1 (ours; opt-in) - SCHEDULE CLASSES: every cloud carries a class and each class its own T0, so clouds that start from
    different times (a tracker's tracked and newly acquired objects) share the launches of one solve (gp_heun_step_classes /
    gp_heun_solve_classes; csrc/pc_rows.h).  run(..., T0=(T0_0 .. T0_{C-1}), eps=, cls=int32 device tensor [B]): all three are run-time
    values refilled in stream order - one capture per geometry.  A row's result is, bit for bit, the uniform sampler's at its class's T0 on
    the same plan and form.  Score model, tile plans: where the automatic layout would take plan 128 the sampler takes the 64-row tiles
    (last_stats['plan']); model='energy', trunk='bf16x9' and tile=128 are refused.  classes=1 is the sampler without classes."""

    LAUNCHES = ("chain", "single")
    MAX_CLASSES = 8  # GP_MAX_SCHED_CLASSES
    # what a solver on the same launch shape, plans and buffers replaces (Dpm2mSampler): the floats per schedule row, the entry points
    # (chain plan on bf16x9, any plan, one launch) and the kernels' names
    SCHED_ROW = 4
    ENTRY = ("gp_heun_step_bf16x9", "gp_heun_step_plan", "gp_heun_solve_tile")
    KERNELS = ("heun_step_chain_kernel", "heun_step_kernel", "heun_solve_kernel")
    ENTRY_CLASSES = ("gp_heun_step_classes", "gp_heun_solve_classes")
    KERNELS_CLASSES = ("heun_step_classes_kernel", "heun_solve_classes_kernel")
    MODELS = ("score", "energy")

    @staticmethod
    def _launches(nsteps, denoise):
        return heun_launches(nsteps, denoise)

    def _schedule(self, T0, eps):
        return heun_schedule(self.n, T0, eps, self.grid, self.rho, self.denoise)

    def _class_schedules(self, T0s, eps):
        """The C-class block: every class's own schedule, stacked - (t [C, N+1], sched [C, launches, row]).  The kind column depends on the
        launch index alone, so it is the same in every class (the kernels read it from class 0)."""
        per = [self._schedule(T0, eps) for T0 in T0s]
        return np.stack([t for t, _ in per]), np.stack([sc for _, sc in per])

    def __init__(self, net, B, K, nsteps, device, groups=1, grid="geometric", rho=7.0, trunk=None, tile=None, record_traj=False, denoise=True,
                 use_graph=True, launches="chain", model="score", classes=1):
        import ctypes
        if not 1 <= int(classes) <= self.MAX_CLASSES:
            raise ValueError(f"classes {classes!r}: 1 .. {self.MAX_CLASSES} schedule classes")
        self.classes = int(classes)
        if self.classes > 1:
            if model == "energy":
                raise ValueError("model='energy' with classes > 1: schedule classes run on the score model's tile kernels")
            if trunk == "bf16x9":
                raise ValueError("trunk='bf16x9' with classes > 1: the split-bf16 trunk is the 128-row chain form, which keeps one time per launch")
            if tile and int(tile) == 128:
                raise ValueError("tile=128 with classes > 1: the 128-row chain form keeps one time per launch; schedule classes run on tiles 16 / 32 / 64")
        if B % groups:
            raise ValueError(f"{B} clouds do not split into {groups} equal batches")
        if grid not in HEUN_GRIDS:
            raise ValueError(f"heun grid {grid!r}: one of {HEUN_GRIDS}")
        if trunk not in (None, "bf16x9", "f32mfma"):
            raise ValueError(f"trunk {trunk!r}: 'bf16x9' or 'f32mfma'")
        if model not in self.MODELS:
            raise ValueError(f"model {model!r}: one of {self.MODELS}")
        if model == "energy" and trunk == "bf16x9":
            raise ValueError("trunk 'bf16x9' with model='energy': the forward + vector-Jacobian pass of the energy model's score has no "
                             "split-bf16 form; use trunk=None or 'f32mfma'")
        self.model = self.MODELS.index(model)
        if tile and int(tile) & _lib.PLAN_HEADSPLIT:
            raise NotImplementedError("the head-split plan has no Heun kernel: whole 16-row tiles serve such sizes (tile=16)")
        if launches not in self.LAUNCHES:
            raise ValueError(f"launches {launches!r}: one of {self.LAUNCHES}")
        self.net, self.B, self.K, self.n, self.groups = net, B, K, int(nsteps), groups
        self.grid, self.rho, self.denoise = grid, float(rho), bool(denoise)
        self.nlaunch = self._launches(self.n, self.denoise)
        self.dev = torch.device(device)
        R = self.R = B * K
        t_out = ctypes.c_int(0)
        if _lib.lib().gp_heun_layout_model(self.model, int(tile or 0), groups, B // groups, K, ctypes.byref(t_out)) != 0:
            raise ValueError(f"{B // groups} clouds x {K} candidates per batch do not split into workgroups of plan {tile or 'auto'}"
                             + (" (the energy model has plans 16 and 128)" if self.model else "") + "; run the batches separately")
        if self.classes > 1 and t_out.value == 128:
            # the automatic layout took the chain form, which has no classes: the 64-row tiles, the next plan of the ladder, serve the size
            if _lib.lib().gp_heun_layout_model(0, 64, groups, B // groups, K, ctypes.byref(t_out)) != 0:
                raise ValueError(f"classes > 1: {B // groups} clouds x {K} candidates per batch take plan 128 and do not split into 64-row tiles; force a tile")
        self.plan = self.tile = t_out.value
        if launches == "single" and self.tile == 128:
            raise ValueError(f"launches='single' serves the tile plans (16 / 32 / 64 rows); {B} clouds x {K} candidates on plan {tile or 'auto'} "
                             "take plan 128, the chain form, which keeps its per-launch kernels: force a tile or use launches='chain'")
        self.launches = launches
        self.trunk = None
        if self.tile == 128:
            self.trunk = "f32mfma" if self.model else trunk or "bf16x9"
            if self.trunk == "bf16x9":
                self._x9 = net.w.bf16x9_packs()
        kc, kt, ks = self.KERNELS
        if self.classes > 1:
            kt, ks = self.KERNELS_CLASSES
        sfx = ",energy>" if self.model else ">"
        self.kernel_name = (f"{kc}<bf16x9>" if self.trunk == "bf16x9" else f"{kc}<2{sfx}" if self.tile == 128
                            else f"{ks}<{self.tile}{sfx}" if launches == "single" else f"{kt}<{self.tile}{sfx}")
        f = lambda *s: torch.empty(*s, device=self.dev)
        self.x, self.d, self.score, self.out = f(R, 9), f(R, 9), f(R, 9), f(R, 9)
        self.cvec, self.centre = f(B, 768), f(B, 3)
        self.traj = f(self.n, R, 9) if record_traj else None
        self._table = _ScheduleTable(net, self.nlaunch, self.SCHED_ROW, self.n + 1, self.dev, classes=self.classes)
        self.sched, self.t_dev, self.tvec_all = self._table.sched, self._table.t_dev, self._table.tvec_all
        self.cls = torch.zeros(B, dtype=torch.int32, device=self.dev) if self.classes > 1 else None  # the class of every cloud (static)
        self.use_graph = use_graph
        self.graph = None
        self.captures = 0
        self.last_stats = {}

    def _write_schedule(self, T0, eps):
        if self.classes > 1:
            T0s = tuple(float(t) for t in (T0 if isinstance(T0, (tuple, list)) else (T0,)))
            if len(T0s) != self.classes:
                raise ValueError(f"T0 {T0!r}: a sampler with {self.classes} schedule classes takes one T0 per class")
            self._table.write((T0s, float(eps)), lambda: self._class_schedules(T0s, eps))
            return
        self._table.write((float(T0), float(eps)), lambda: self._schedule(T0, eps))

    def launch_step(self, l):
        """Launch l of the chain (0 <= l < nlaunch) on the current stream."""
        shape = (self.groups, self.B // self.groups, self.K, l, self.n, int(self.denoise))
        bufs = (ptr(self.cvec), ptr(self.tvec_all), ptr(self.sched), ptr(self.centre), ptr(self.x), ptr(self.d), ptr(self.score), ptr(self.out),
                ptr(self.traj))
        if self.classes > 1:
            _lib.call(self.ENTRY_CLASSES[0], 0, self.plan, *shape, self.net.w.ref(), *bufs, self.classes, ptr(self.cls), stream_ptr())
        elif self.trunk == "bf16x9":
            _lib.call(self.ENTRY[0], *shape, self.net.w.ref(), *bufs, *(ptr(w) for w in self._x9), stream_ptr())
        elif self.model:
            _lib.call(self.ENTRY[1] + "_model", self.model, self.plan, *shape, self.net.w.ref(), *bufs, stream_ptr())
        else:
            _lib.call(self.ENTRY[1], self.plan, *shape, self.net.w.ref(), *bufs, stream_ptr())

    def _launch_all(self):
        if self.launches == "single" and self.classes > 1:
            _lib.call(self.ENTRY_CLASSES[1], 0, self.plan, self.groups, self.B // self.groups, self.K, self.n, int(self.denoise), self.net.w.ref(),
                      ptr(self.cvec), ptr(self.tvec_all), ptr(self.sched), ptr(self.centre), ptr(self.x), ptr(self.d), ptr(self.score), ptr(self.out),
                      ptr(self.traj), self.classes, ptr(self.cls), stream_ptr())
            return
        if self.launches == "single":
            _lib.call(*((self.ENTRY[2] + "_model", self.model) if self.model else (self.ENTRY[2],)), self.plan, self.groups, self.B // self.groups, self.K, self.n, int(self.denoise), self.net.w.ref(),
                      ptr(self.cvec), ptr(self.tvec_all), ptr(self.sched), ptr(self.centre), ptr(self.x), ptr(self.d), ptr(self.score), ptr(self.out),
                      ptr(self.traj), stream_ptr())
            return
        for l in range(self.nlaunch):
            self.launch_step(l)

    def run(self, cvec, centre, x0, T0=1.0, eps=EPS, cls=None):
        """cvec [B,768], centre [B,3], x0 [R,9] (the state at T0).  Returns (xs [R,N,9] or None, pose [R,9]) float32: x_1 .. x_N and the
        final pose, rotations normalised and cloud centres added.  With schedule classes: T0 one per class, cls [B] int32 on the device,
        x0 every cloud's state at its class's T0."""
        if cvec.shape[0] != self.B or x0.shape[0] != self.R:
            raise ValueError(f"Heun sampler set up for {self.B} clouds x {self.K} candidates got {cvec.shape[0]} clouds / {x0.shape[0]} rows")
        if (cls is not None) != (self.classes > 1):
            raise ValueError("cls= goes with a sampler built with classes > 1" if cls is not None else f"a sampler with {self.classes} schedule classes needs cls=")
        if cls is not None:
            if cls.dtype != torch.int32 or tuple(cls.shape) != (self.B,):
                raise ValueError(f"cls: int32 [{self.B}], got {cls.dtype} {tuple(cls.shape)}")
            self.cls.copy_(cls)
        self.cvec.copy_(cvec)
        self.centre.copy_(centre)
        self.x.copy_(x0)
        self._write_schedule(T0, eps)
        if not self.use_graph:
            self._launch_all()
        else:
            _replay_captured(self, x0)
        self.last_stats = {"nfev": self.nlaunch - 1, "plan": self.plan, "launches": self.nlaunch, "kernel": self.kernel_name,
                           "nlaunch": self.nlaunch, "kernel_name": self.kernel_name}
        if self.launches == "single":
            self.last_stats["device_launches"] = 1
        xs = self.traj.permute(1, 0, 2) if self.traj is not None else None
        return xs, self.out


# ---------------------------------------------------------------------------------------------- PF-ODE (fixed-step DPM-Solver++(2M))
DPM2M_SCHED_ROW = 8


def dpm2m_launches(nsteps, denoise=True):
    """Launches of a DPM-Solver++(2M) chain (gp_dpm2m_launches): N + 1, one more with denoise.  NFE = launches - 1."""
    if int(nsteps) < 1:
        raise ValueError(f"nsteps {nsteps}: at least one step")
    return int(nsteps) + 1 + (1 if denoise else 0)


def dpm2m_coefficients(sig):
    """Per step i = 0 .. N-1 of DPM-Solver++(2M) on the sigma grid `sig` [N+1] (float64): sigma_i^2, sigma_{i+1} / sigma_i and the weights
    of D_i and D_{i-1} times -expm1(-h_i), with lambda = -ln sigma, h_i = lambda_{i+1} - lambda_i, r_i = (lambda_i - lambda_{i-1}) / h_i:
    wc = -expm1(-h_i) (1 + 1/(2 r_i)), wp = -expm1(-h_i) (-1/(2 r_i)); step 0 is first order (wc = -expm1(-h_0), wp = 0).  float64."""
    sig = np.asarray(sig, dtype=np.float64)
    lam = -np.log(sig)
    h = lam[1:] - lam[:-1]
    em = -np.expm1(-h)
    wc, wp = em.copy(), np.zeros_like(em)
    for i in range(1, len(h)):
        r = (lam[i] - lam[i - 1]) / h[i]
        wc[i] = em[i] * (1.0 + 1.0 / (2.0 * r))
        wp[i] = em[i] * (-(1.0 / (2.0 * r)))
    return sig[:-1] * sig[:-1], sig[1:] / sig[:-1], wc, wp


def dpm2m_schedule(nsteps, T0=1.0, eps=EPS, grid="geometric", rho=7.0, denoise=True):
    """Host schedule of a DPM-Solver++(2M) chain on heun_schedule's grid: (t [N+1] f64, sched [launches,8] f32) - per launch the sigma of
    its evaluation (the score's divisor), sigma_{i-1}^2, sigma_i / sigma_{i-1}, the launch kind, the two denoiser weights already multiplied
    by -expm1(-h) and two zeros (include/genpose_hip.h: gp_dpm2m_step_plan), computed in float64 and rounded once.  Launch l evaluates at
    t_l; the denoising launch carries g(eps) and the predictor's step where the steps carry sigma^2 and the ratio."""
    N = int(nsteps)
    t, sig = heun_grid(N, T0, eps, grid, rho)
    s2, ratio, wc, wp = dpm2m_coefficients(sig)
    sched = np.zeros((dpm2m_launches(N, denoise), DPM2M_SCHED_ROW), dtype=np.float64)
    sched[0, 0] = sig[0]
    for i in range(N):
        sched[i + 1, :6] = (sig[i + 1], s2[i], ratio[i], 3.0 if i == N - 1 else 2.0, wc[i], wp[i])
    if denoise:
        # the reverse-diffusion predictor at eps (samplers.py:209-218) with cond_ode_sampler's divisor rule for num_steps = N, as heun_schedule
        g = np.float32(sig[N]) * _HEUN_G_FACTOR
        sched[N + 1, :4] = (sig[N], g, (1.0 - float(eps)) / N, 4.0)
    return t, sched.astype(np.float32)


class Dpm2mSampler(HeunSampler):
    """Fixed-step DPM-Solver++(2M) solver of the probability-flow ODE (ours; opt-in): the second-order multistep exponential integrator in
    lambda = -ln sigma on the denoiser D = x + sigma^2 score - ONE evaluation per step, the previous step's denoiser carried along, the
    linear part of the VE flow integrated exactly; state in fp32.  NFE = N (+ 1 with denoise) in N + 1 (+ 1) launches against HeunSampler's
    2 N (+ 1) on the same grid.  Everything else is HeunSampler's: constructor, plans, trunk, buffers (d holds the previous denoiser),
    run-time T0 / eps with one capture per geometry, launches 'chain' | 'single' (gp_dpm2m_solve_tile), row locality, the finish (denoise,
    normalize_rotation, cloud centre) and the trajectory's layout."""

    SCHED_ROW = DPM2M_SCHED_ROW
    ENTRY = ("gp_dpm2m_step_bf16x9", "gp_dpm2m_step_plan", "gp_dpm2m_solve_tile")
    KERNELS = ("dpm2m_step_chain_kernel", "dpm2m_step_kernel", "dpm2m_solve_kernel")
    ENTRY_CLASSES = ("gp_dpm2m_step_classes", "gp_dpm2m_solve_classes")
    KERNELS_CLASSES = ("dpm2m_step_classes_kernel", "dpm2m_solve_classes_kernel")

    @staticmethod
    def _launches(nsteps, denoise):
        return dpm2m_launches(nsteps, denoise)

    def _schedule(self, T0, eps):
        return dpm2m_schedule(self.n, T0, eps, self.grid, self.rho, self.denoise)


# ---------------------------------------------------------------------------------------------- likelihood ODE (fixed-step Heun)
def heun_likelihood_launches(nsteps):
    """Launches of a Heun likelihood chain (gp_heun_likelihood_launches): 2 N + 1.  NFE = 2 N."""
    if int(nsteps) < 1:
        raise ValueError(f"nsteps {nsteps}: at least one step")
    return 2 * int(nsteps) + 1


def heun_likelihood_schedule(nsteps, eps=EPS, T=1.0, grid="geometric", rho=7.0):
    """Host schedule of a Heun solve of the likelihood ODE, which runs from eps UP to T: (t [N+1] f64 ascending, sched [2N+1,4] f32).  The
    times are heun_grid's points in ascending order (they end exactly at eps and T); per launch the sigma of its evaluation, the factor
    c = -sigma, the step h = sigma_{i+1} - sigma_i > 0 and the launch kind (include/genpose_hip.h: gp_heun_likelihood_step), computed in
    float64 and rounded once."""
    N = int(nsteps)
    t, sig = heun_grid(N, T, eps, grid, rho)
    t, sig = np.ascontiguousarray(t[::-1]), np.ascontiguousarray(sig[::-1])
    h = sig[1:] - sig[:-1]
    sched = np.zeros((heun_likelihood_launches(N), 4), dtype=np.float64)
    sched[0] = (sig[0], 0.0, 0.0, 0.0)
    for i in range(N):
        sched[2 * i + 1] = (sig[i + 1], -sig[i], h[i], 1.0)
        sched[2 * i + 2] = (sig[i + 1], -sig[i + 1], h[i], 2.0)
    sched[2 * N, 3] = 3.0
    return t, sched.astype(np.float32)


class HeunLikelihood:
    """Fixed-step Heun solve of the likelihood ODE with the exact divergence (cond_ode_likelihood's system, samplers.py:22-99), integrated
    in sigma from sigma(eps) up to sigma(T) on heun_schedule's grids: x and the slopes in fp32, the log-density change in float64
    (csrc/heun_likelihood.hip).  Deterministic, fixed NFE = 2 N, ROW-LOCAL: the value of (cloud, pose) is a function of (cloud, pose, N, grid,
    eps) alone, bit for bit, whatever else shares the call.  One captured chain of 2 N + 1 launches per geometry, nothing read back; eps is a
    run-time value (the schedule and the time-embedding table are device buffers refilled in stream order), so a new eps never recaptures.
    16-row tiles only."""

    def __init__(self, net, B, K, device, nsteps, grid="geometric", rho=7.0, use_graph=True):
        if grid not in HEUN_GRIDS:
            raise ValueError(f"heun grid {grid!r}: one of {HEUN_GRIDS}")
        self.net, self.B, self.K, self.n = net, B, K, int(nsteps)
        self.grid, self.rho = grid, float(rho)
        self.nlaunch = heun_likelihood_launches(self.n)
        self.dev = torch.device(device)
        R = self.R = B * K
        self.kernel_name = "heun_likelihood_step_kernel"
        f = lambda *s: torch.empty(*s, device=self.dev)
        self.x, self.d, self.score, self.div, self.z = f(R, 9), f(R, 10), f(R, 9), f(R), f(R, 9)
        self.logp = torch.zeros(R, dtype=torch.float64, device=self.dev)
        self.cvec = f(B, 768)
        self._table = _ScheduleTable(net, self.nlaunch, 4, self.n + 1, self.dev)
        self.sched, self.t_dev, self.tvec_all = self._table.sched, self._table.t_dev, self._table.tvec_all
        self.use_graph = use_graph
        self.graph = None
        self.captures = 0
        self.last_stats = {}

    def _write_schedule(self, eps, T):
        self._table.write((float(eps), float(T)), lambda: heun_likelihood_schedule(self.n, eps, T, self.grid, self.rho))

    def launch_step(self, l):
        """Launch l of the chain (0 <= l < nlaunch) on the current stream."""
        _lib.call("gp_heun_likelihood_step", self.B, self.K, l, self.n, self.net.w.ref(), ptr(self.cvec), ptr(self.tvec_all), ptr(self.sched),
                  ptr(self.x), ptr(self.d), ptr(self.score), ptr(self.div), ptr(self.logp), ptr(self.z), stream_ptr())

    def _launch_all(self):
        for l in range(self.nlaunch):
            self.launch_step(l)

    def run(self, cvec, x, eps=EPS, T=1.0):
        """cvec [B,768], x [R,9] (the poses whose likelihood is wanted, the state at eps).  Returns (z [R,9] f32: x at T, delta_logp [R] f64)
        on the device - the solver's own buffers, which the next run overwrites."""
        if cvec.shape[0] != self.B or x.shape[0] != self.R:
            raise ValueError(f"Heun likelihood solver set up for {self.B} clouds x {self.K} candidates got {cvec.shape[0]} clouds / {x.shape[0]} rows")
        self.cvec.copy_(cvec)
        self.x.copy_(x)
        self._write_schedule(eps, T)
        if not self.use_graph:
            self._launch_all()
        else:
            _replay_captured(self, x)
        self.last_stats = {"nfev": self.nlaunch - 1, "launches": self.nlaunch, "kernel": self.kernel_name, "n_attempts": self.n}
        return self.z, self.logp


# ---------------------------------------------------------------------------------------------- PF-ODE (RK45)
_STATE_FIELDS = ("t", "h_abs", "status", "n_attempts", "n_accepted", "nfev", "err_norm", "log_t", "log_h", "log_err", "log_acc",
                 "stage_t", "last_accepted")


def _state_layout():
    import ctypes
    arr = (ctypes.c_int64 * 16)()
    _lib.call("gp_rk45_state_layout", arr, 16)
    return {n: int(arr[i]) for i, n in enumerate(_STATE_FIELDS)}, int(_lib.lib().gp_rk45_state_bytes())


class ODESampler:
    """cond_ode_sampler (samplers.py:163-227) with the whole Dormand-Prince loop resident on the GPU.

    One *attempt* (stage-time embedding + 6 fused stage kernels + controller) is captured as a hipGraph and replayed;
    the host only polls the device-side `status` word every `poll` attempts (the number of attempts is data dependent:
    scipy's adaptive controller, rtol = atol = 1e-5, batch-global RMS error norm)."""

    TRAJ_CAP = 192
    CHUNKS = (8, 12, 16, 24, 32, 40, 48, 64, 80, 96, 128)  # attempts per first replay

    MAX_GRAPHS = 12  # captured attempt graphs kept per kind (each holds chunk x 8 kernel nodes)
    MODELS = {"score": 0, "energy": 1, "likelihood": 2, "likelihood_exact": _lib.RK45_MODEL_LIKELIHOOD_EXACT}
    LIKELIHOOD_MODELS = (2, _lib.RK45_MODEL_LIKELIHOOD_EXACT)  # ten state components per row: pose + log-density change

    def __init__(self, net, B, K, device, use_graph=True, poll=8, groups=1, group_clouds=None, model="score", coupling_group=None, tile=0,
                 trunk=None):
        """B clouds in `groups` independent batches of B/groups clouds laid out back to back: every batch keeps its own adaptive
        step control (error norm over ITS rows, accept / reject, step size - what separate cond_ode_sampler calls would do) while
        all of them share each launch (gp_rk45_phase_model).

        model: what the driver integrates (gp_rk45_phase_model) - 'score' the probability-flow ODE of the score network; 'energy' the
        same ODE with the ENERGY network's score (`net` holds its weights; forward + vector-Jacobian product inside the stage
        kernels); 'likelihood' the [pose, log-density] ODE of cond_ode_likelihood (run_likelihood) with its one-probe Hutchinson
        divergence; 'likelihood_exact' the same ODE with the exact divergence tr(d score / d x) (nine unit seeds per row inside the stage
        kernel, csrc/score_bwd.h: no probe, 16-row tiles only).

        coupling_group (a torch.distributed process group; "faithful" multi-GPU mode, SURVEY §8e caveat): this rank's B clouds are one
        SHARD of a batch spread over the ranks of the group (equal shards).  scipy's error norm - and the norms of its initial-step
        heuristic - run over the WHOLE batch: after the stage kernels the per-group sums of squares are all-reduced (two doubles per
        group) and the step controller decides on the reduced sums, so every shard takes the accept / reject sequence of the unsharded
        batch.  On RCCL the all-reduce is captured with the attempts; on gloo the attempts run launch by launch.

        tile: launch plan of the stage kernels (0 = pick: 16- / 32-row tiles, or the 128-row chain form of the trunk for score-model
        launches of ~32 000 rows and more, gp_rk45_plan_rows); tests and measurements force one.

        trunk: the arithmetic of the score model's chain plan (128 rows per workgroup, equal groups) - None / 'f32mfma' (the default: the
        fp32 MFMA stage kernels) or 'bf16x9' (OPT-IN; csrc/rk45.hip: rk45_stage_chain_kernel_bf16x9 - the dense layers as exact-product
        split bf16 on the BF16 matrix pipe, fp32 accuracy; gp_rk45_phase_bf16x9).  It does not touch the choice of plan and is ignored
        under every other plan or model; `self.trunk` holds the effective value."""
        if trunk not in (None, "f32mfma", "bf16x9"):
            raise ValueError(f"trunk {trunk!r}: 'f32mfma' or 'bf16x9'")
        self.model = self.MODELS[model]
        self.ncomp = 10 if self.model in self.LIKELIHOOD_MODELS else 9
        self.ragged = group_clouds is not None
        self.shared = False
        if self.ragged and self.model != 0:
            raise NotImplementedError("ragged groups integrate the score network's ODE only")
        self.dev = torch.device(device)
        if self.ragged:
            # groups of different sizes (tracking: the objects of one frame): consecutive cloud ranges, tiles that end at the group
            # boundary (gp_rk45_phase_ragged).  B and len(group_clouds) are CAPACITIES: set_groups() re-fills the device tables for
            # any grouping that fits, so the captured graphs (fixed grids) serve frames whose object counts change.
            groups = len(group_clouds)
            self.tile = (int(tile) & ~_lib.PLAN_HEADSPLIT) if tile else _lib.lib().gp_score_tile_rows(B * K)  # 16 rows, or 32 once the launch is MFMA-bound
            if self.tile not in (16, 32):
                raise ValueError("ragged groups run on 16- or 32-row tiles")
            self.nblocks = (B * K + self.tile - 1) // self.tile + groups  # every group wastes less than one tile
            # latency regime (one sequence's frames: a few dozen tiles at capacity): three workgroups per tile, one head of the network each
            if tile:
                self.hsplit = 3 if int(tile) & _lib.PLAN_HEADSPLIT else 1
            else:
                self.hsplit = 3 if self.tile == 16 and _lib.lib().gp_plan_headsplit_pays(self.nblocks) else 1
            self.plan = self.tile | (_lib.PLAN_HEADSPLIT if self.hsplit == 3 else 0)
            self.blk_info = torch.zeros(self.nblocks, 3, dtype=torch.int32, device=self.dev)
            self.grp_info = torch.zeros(groups, 4, dtype=torch.int32, device=self.dev)
            self._tables_host = (torch.zeros(self.nblocks, 3, dtype=torch.int32).pin_memory(), torch.zeros(groups, 4, dtype=torch.int32).pin_memory())
        elif B % groups:
            raise ValueError(f"{B} clouds do not split into {groups} equal batches")
        self.net, self.B, self.K, self.groups = net, B, K, groups
        R = self.R = B * K
        if not self.ragged:
            # forward + backward right-hand sides (energy model, likelihood): 16-row tiles or, for large launches, the 128-row chain form
            # (a sharded batch's controller runs on all-reduced per-group sums between the stage launches and the decision: not the shared-chunk plan)
            pick = _lib.lib().gp_rk45_plan_rows if coupling_group is None else _lib.lib().gp_rk45_plan_rows_unshared
            self.plan = int(tile) if tile else pick(self.model, groups, B // groups, K)
            # plan = rows per workgroup | GP_PLAN_HEADSPLIT (three workgroups per 16-row tile, one head each - the latency regime)
            #                           | GP_PLAN_SHARED (one workgroup per CU, the left-over 16-row chunks shared across the stages of an attempt)
            self.tile, self.hsplit = self.plan & ~_lib.PLAN_FLAGS, (3 if self.plan & _lib.PLAN_HEADSPLIT else 1)
            self.shared = bool(self.plan & _lib.PLAN_SHARED)
            if self.model == _lib.RK45_MODEL_LIKELIHOOD_EXACT and self.plan != 16:
                raise ValueError(f"model 'likelihood_exact' runs on 16-row tiles (plan {self.plan:#x}; several batches: rows per batch a multiple of 16)")
            if ((self.hsplit == 3 and (self.tile != 16 or self.model != 0)) or self.tile not in (16, 32, 48, 64, 128) or (self.tile == 48 and not self.shared)
                    or (self.model != 0 and self.tile in (32, 48, 64)) or (groups > 1 and (R // groups) % self.tile)):
                raise ValueError(f"{B // groups} clouds x {K} candidates per batch do not split into workgroups of plan {tile or 'auto'}; "
                                 "run the batches separately")
            npart = _lib.lib().gp_rk45_partials_count(self.model, self.plan, groups, B // groups, K)
            if npart <= 0:
                raise ValueError(f"plan {self.plan:#x} does not serve {groups} x {B // groups} clouds x {K} candidates")
            self.nblocks = npart // (3 * self.hsplit)
        self.trunk = "f32mfma"
        if trunk == "bf16x9" and not self.ragged and self.model == 0 and self.plan == 128:
            self.trunk = "bf16x9"
            self._x9 = net.w.bf16x9_packs()
        if self.trunk == "bf16x9":
            self.kernel_name = "rk45_stage_chain_kernel<bf16x9>"
        elif self.shared:
            self.kernel_name = f"rk45_attempt_shared_kernel<{self.tile}>"
        elif self.tile == 128:
            self.kernel_name = "rk45_stage_chain_kernel<2>" if self.model == 0 else f"rk45_stage_chain_kernel<2,{model}>"
        elif self.hsplit == 3:
            self.kernel_name = "rk45_stage_kernel<16,split>"
        elif self.tile == 16:
            self.kernel_name = "rk45_attempt_kernel<16>" if self.model == 0 else f"rk45_attempt_kernel<16,{model}>"
        else:
            self.kernel_name = f"rk45_stage_kernel<{self.tile}>"
        if self.ragged:
            self.set_groups(group_clouds)
        self.layout, nbytes = _state_layout()
        self.state_bytes = nbytes
        self.state = torch.zeros(groups * nbytes, dtype=torch.uint8, device=self.dev)
        d = lambda *s: torch.zeros(*s, dtype=torch.float64, device=self.dev)
        nc = self.ncomp
        self.y, self.ynew, self.Kbuf = d(R * nc), d(R * nc), d(7, R * nc)
        self.partials = d(3, self.nblocks * self.hsplit)
        self.x_out = d(R, nc)
        self.probe = torch.zeros(R, 9, device=self.dev) if self.model == 2 else None
        self.coupling_group, self.ext_sums, self.ext_rows = coupling_group, None, 0
        if coupling_group is not None:
            if self.ragged:
                raise NotImplementedError("ragged groups are not sharded")
            import torch.distributed as dist
            self._dist = dist
            self.ext_sums = d(2, groups)
            self.ext_rows = R // groups * dist.get_world_size(coupling_group)
            use_graph = use_graph and dist.get_backend(coupling_group) == "nccl"
        self.tvec = torch.zeros(groups * 8, 768, device=self.dev)
        self.cvec = torch.empty(B, 768, device=self.dev)
        self.centre = torch.empty(B, 3, device=self.dev)
        self.traj = None
        if self.model in self.LIKELIHOOD_MODELS and poll == 8:
            poll = 64  # the likelihood ODE runs from eps to 1 at rtol 1e-5: thousands of attempts, fewer status reads
        self.use_graph, self.poll = use_graph, poll
        self._graphs = {}        # kind ('graph' | 'graph_traj' | 'graph_dense') -> {attempts per replay: captured graph}
        self._attempt_hist = {}  # (kind, T0) -> attempts the previous solve took
        self.last_stats = {}

    def set_groups(self, group_clouds):
        """Ragged mode: (re)define the groups - clouds per group, consecutive; fewer groups / clouds than the capacity leave padding
        workgroups and padding groups that exit at once.  Returns the number of clouds in use."""
        group_clouds = [int(c) for c in group_clouds]
        if len(group_clouds) > self.groups or sum(group_clouds) > self.B or (group_clouds and min(group_clouds) <= 0):
            raise ValueError(f"groups {group_clouds} exceed the capacity ({self.groups} groups, {self.B} clouds)")
        blk_h, grp_h = self._tables_host
        # the pinned host tables are rewritten below: only the previous upload out of them has to be complete (the device
        # tables themselves are overwritten in stream order, behind every launch that still reads them)
        if getattr(self, "_tables_ev", None) is not None:
            self._tables_ev.synchronize()
        blk, grp = blk_h.numpy(), grp_h.numpy()
        blk[:] = 0
        grp[:] = 0
        if group_clouds:
            rows = np.asarray(group_clouds, dtype=np.int64) * self.K
            nb = (rows + self.tile - 1) // self.tile
            row0 = np.concatenate([[0], np.cumsum(rows)[:-1]])
            blk0 = np.concatenate([[0], np.cumsum(nb)[:-1]])
            ng = len(group_clouds)
            grp[:ng] = np.stack([blk0, nb, rows, row0], axis=1)
            gid = np.repeat(np.arange(ng), nb)
            local = np.arange(int(nb.sum())) - np.repeat(blk0, nb)
            blk[: len(gid)] = np.stack([gid, row0[gid] + local * self.tile, (row0 + rows)[gid]], axis=1)
        self.blk_info.copy_(blk_h, non_blocking=True)
        self.grp_info.copy_(grp_h, non_blocking=True)
        if getattr(self, "_tables_ev", None) is None:
            self._tables_ev = torch.cuda.Event()
        self._tables_ev.record(torch.cuda.current_stream(self.dev))
        self.group_clouds = group_clouds
        return sum(group_clouds)

    def _phase(self, phase, traj=None, t0=0.0, t_bound=0.0, rtol=1e-5, atol=1e-5, dscale=0.0, do_denoise=1, nstates=0):
        import ctypes
        cd = ctypes.c_double
        # every entry point takes: its own head, the phase, its geometry, the solver's buffers (_lib.RK45_SOLVE), its own tail, the stream
        fn, head, tail = "gp_rk45_phase_ragged", (), ()
        if self.ragged:
            geom = (self.groups, ptr(self.grp_info), self.nblocks, ptr(self.blk_info), self.plan, self.B, self.K)
        else:
            geom, tail = (self.groups, self.B // self.groups, self.K), (ptr(self.ext_sums), self.ext_rows)
            if self.trunk == "bf16x9":
                fn, tail = "gp_rk45_phase_bf16x9", tail + tuple(ptr(w) for w in self._x9)
            else:
                fn, head = "gp_rk45_phase_model", (self.model, self.plan, ptr(self.probe))
        solve = (*geom, self.net.w.ref(), ptr(self.cvec), ptr(self.tvec), ptr(self.centre), ptr(self.state), ptr(self.y), ptr(self.ynew), ptr(self.Kbuf),
                 ptr(self.partials), ptr(traj), 0 if traj is None else traj.shape[0], cd(t0), cd(t_bound), cd(rtol), cd(atol), cd(dscale), do_denoise,
                 nstates, ptr(self.x_out), *tail, stream_ptr())
        _lib.call(fn, *head, phase, *solve)
        if self.ext_sums is not None and not self.ragged and phase in (1, 2, 3):
            # sharded batch: the controller decides on the sums of squares over ALL shards
            self._dist.all_reduce(self.ext_sums, op=self._dist.ReduceOp.SUM, group=self.coupling_group)
            _lib.call(fn, *head, phase + 10, *solve)

    def _attempt(self, traj):
        # the step controller at the end of phase 3 (and of phase 2 before the first attempt) also writes the time embeddings of the
        # next attempt's six stage times: an attempt is six stage launches + one controller launch
        self._phase(3, traj)

    def _read_states(self):
        if getattr(self, "_state_host", None) is None:
            self._state_host = torch.empty(self.state.shape, dtype=torch.uint8).pin_memory()
        self._state_host.copy_(self.state, non_blocking=True)  # one D2H copy for all groups, into pinned memory
        torch.cuda.current_stream(self.dev).synchronize()
        raw_all = self._state_host.numpy()
        return [self._parse_state(raw_all[g * self.state_bytes:(g + 1) * self.state_bytes]) for g in range(self.groups)]

    def _read_state(self, group=0):
        return self._read_states()[group]

    def _parse_state(self, raw):
        L = self.layout
        g = lambda name, dt, n=1: np.frombuffer(raw.tobytes(), dtype=dt, count=n, offset=L[name])
        st = {k: g(k, np.int32)[0] for k in ("status", "n_attempts", "n_accepted", "nfev")}
        st.update({k: g(k, np.float64)[0] for k in ("t", "h_abs", "err_norm")})
        na = min(int(st["n_attempts"]), 512)
        st["log_t"], st["log_h"], st["log_err"] = (g(k, np.float64, 512)[:na].copy() for k in ("log_t", "log_h", "log_err"))
        st["log_acc"] = g("log_acc", np.int32, 512)[:na].copy()
        return st

    def _solve(self, traj, gname, T0, max_attempts=4096):
        """The adaptive loop after phases 0-2: replays captured attempts until every group's device-side status word is set.
        Returns the per-group states."""
        n_done = 0
        # The attempt count is data dependent (scipy's controller), but it barely moves between solves of the same kind (same T0, same
        # kind of clouds), and an attempt launched on a FINISHED solve exits at once.  So the first replay is a graph sized for the
        # previous solve's attempt count (+ margin): in the common case the whole adaptive loop is ONE graph replay and one status
        # read; a solve that needs more continues in chunks of `poll` attempts.
        hist_key = (gname, round(float(T0), 3))
        expect = self._attempt_hist.get(hist_key)
        # (solves of up to 64 attempts - tracking: 6-8, the benched ODE-100: 36 - get a graph of exactly one spare attempt: every attempt
        # launched on a finished solve is eight kernels that exit at once, ~35 us, and a coarse chunk list made 12 attempts out of 7)
        first = self.poll if expect is None else (expect + 1 if expect < 64 else next((c for c in self.CHUNKS if c >= expect + 2), self.CHUNKS[-1]))
        if expect is not None and expect < 64 and self.use_graph:
            # a solve whose attempt count drifts by one or two from frame to frame must not pay a capture (torch.cuda.graph synchronises
            # the device) in the middle of a latency-critical frame: take an already captured graph with up to three more spare attempts
            # (each is eight kernels that exit at once) before capturing a new size
            have = [c for c in self._graphs.get(gname, {}) if first <= c <= first + 3]
            if have:
                first = min(have)
        while True:
            chunk = first if n_done == 0 else self.poll
            if self.use_graph:
                graphs = self._graphs.setdefault(gname, {})
                if chunk not in graphs:
                    if not graphs:
                        self._attempt(traj)  # warm-up outside capture
                        n_done += 1
                    graphs[chunk] = capture(lambda: [self._attempt(traj) for _ in range(chunk)]).graph
                    if len(graphs) > self.MAX_GRAPHS:  # bounded cache: drop the least recently captured size that is not in use now
                        for c in list(graphs):
                            if c not in (chunk, self.poll):
                                del graphs[c]
                                break
                graphs[chunk].replay()
            else:
                for _ in range(chunk):
                    self._attempt(traj)
            n_done += chunk
            sts = self._read_states()
            if self.ragged:
                sts = sts[: len(self.group_clouds)]
            if all(s_["status"] != 0 for s_ in sts):
                break
            if n_done >= max_attempts:
                raise RuntimeError("ODE sampler: attempt budget exhausted")
        if any(s_["status"] == -2 for s_ in sts):
            raise RuntimeError("ODE sampler: a stage of the shared-chunk plan never saw its predecessor's state (bounded wait ran out); "
                               "force a whole-tile plan with ODESampler(..., tile=64)")
        if any(s_["status"] < 0 for s_ in sts):
            raise RuntimeError("ODE sampler: required step size is less than spacing between numbers (scipy TOO_SMALL_STEP)")
        self.group_stats = sts
        self._attempt_hist[hist_key] = max(int(s_["n_attempts"]) for s_ in sts)
        self.last_replays = {"first_chunk": first, "attempts_launched": n_done}
        return sts

    def run_likelihood(self, cvec, x, probe=None, eps=EPS, rtol=1e-5, atol=1e-5, max_attempts=16384):
        """cond_ode_likelihood's integration (samplers.py:73-93) on the device: state [x, logp] from t = eps to t = 1 with the fixed
        Hutchinson probe (model 'likelihood') or the exact divergence (model 'likelihood_exact': probe must be None).  cvec [B,768];
        x, probe [B*K,9].  Returns (z [R,9] f64, delta_logp [R] f64); evaluation count in last_stats['nfev'] (2 for the initial step +
        6 per attempt, like solve_ivp)."""
        if self.model not in self.LIKELIHOOD_MODELS:
            raise RuntimeError("ODESampler(model='likelihood' | 'likelihood_exact') required")
        exact = self.model != 2
        if exact and probe is not None:
            raise ValueError("model 'likelihood_exact' takes no probe: its divergence is the exact trace")
        if not exact and probe is None:
            raise ValueError("model 'likelihood' needs the Hutchinson probe [B*K,9]")
        R = self.R
        if cvec.shape[0] != self.B or x.shape[0] != R or (probe is not None and probe.shape[0] != R):
            raise ValueError(f"likelihood solver set up for {self.B} clouds x {self.K} rows got {cvec.shape[0]} clouds / {x.shape[0]} rows")
        self.cvec.copy_(cvec)
        self.centre.zero_()
        if not exact:
            self.probe.copy_(probe.float())
        y0 = self.y.view(R, 10)
        y0[:, :9].copy_(x.double())   # solve_ivp casts the initial state to float64
        y0[:, 9].zero_()
        self._phase(0, None, t0=eps, t_bound=1.0, rtol=rtol, atol=atol)
        self._phase(1, None)
        self._phase(2, None)
        sts = self._solve(None, "graph", eps, max_attempts)
        self._phase(5, None)
        self.last_stats = sts[0]
        out = self.x_out.clone()
        return out[:, :9], out[:, 9]

    def run(self, cvec, centre, init_x, T0, num_steps=None, eps=EPS, rtol=1e-5, atol=1e-5, denoise=True, return_process=False,
            max_attempts=4096):
        """Returns (xs [R,S,9] f64 or None, x [R,9] f64).  With num_steps=None the in-process samples are the accepted
        states (like solve_ivp without t_eval)."""
        if self.model in self.LIKELIHOOD_MODELS:
            raise RuntimeError("ODESampler(model='likelihood') integrates the likelihood ODE: call run_likelihood()")
        dense = return_process and num_steps is not None
        if self.groups > 1 and return_process and not dense:
            raise NotImplementedError("accepted-state trajectories have a different length per batch: ask for them one batch at a time")
        nb_in = cvec.shape[0]  # ragged mode may use fewer clouds than the capacity
        expect = sum(self.group_clouds) if self.ragged else self.B
        if nb_in != expect or init_x.shape[0] != nb_in * self.K:
            raise ValueError(f"ODE sampler set up for {expect} clouds x {self.K} candidates got {nb_in} clouds / {init_x.shape[0]} rows"
                             + (" (call set_groups() with this step's grouping first)" if self.ragged else ""))
        self.cvec[:nb_in].copy_(cvec)
        self.centre[:nb_in].copy_(centre)
        self.y[: nb_in * self.K * 9].copy_(init_x.reshape(-1))  # init_x f32 -> f64 state in the copy (solve_ivp casts y0 to float64)
        traj = None
        if dense:
            # solve_ivp(t_eval=np.linspace(T0, eps, num_steps)): 4th-order dense output at every t_eval point
            import ctypes
            from scipy.integrate._ivp.rk import RK45  # published dense-output constants (7x4 matrix P)
            key = ("dense", num_steps)
            if getattr(self, "_dense_key", None) != key:
                self._dense_traj = torch.zeros(num_steps, self.R * 9, dtype=torch.float64, device=self.dev)
                self._dense_key = key
                self._graphs.pop("graph_dense", None)  # the captured attempts hold the trajectory pointer
            self._t_eval = torch.from_numpy(np.linspace(T0, eps, num_steps)).to(self.dev)
            traj = self._dense_traj
            self._phase(0, None, t0=T0, t_bound=eps, rtol=rtol, atol=atol)
            Pm = np.ascontiguousarray(RK45.P, dtype=np.float64)
            _lib.call("gp_rk45_set_dense_grouped", self.groups, ptr(self.state), ptr(self._t_eval), num_steps, Pm.ctypes.data_as(ctypes.c_void_p),
                      stream_ptr())
        else:
            if return_process:
                if self.traj is None:
                    self.traj = torch.zeros(self.TRAJ_CAP, self.R * 9, dtype=torch.float64, device=self.dev)
                traj = self.traj
            self._phase(0, traj, t0=T0, t_bound=eps, rtol=rtol, atol=atol)
        self._phase(1, traj)
        self._phase(2, traj)
        gname = "graph_dense" if dense else ("graph_traj" if traj is not None else "graph")
        sts = self._solve(traj, gname, T0, max_attempts)
        st = sts[0]
        self._phase(4, traj, t0=eps)
        nstates = (num_steps if dense else int(st["n_accepted"]) + 1) if traj is not None else 0
        if traj is not None and not dense and nstates > self.TRAJ_CAP:
            self._attempt_hist.pop((gname, round(float(T0), 3)), None)  # a failed solve leaves no attempt-count expectation behind
            raise RuntimeError(f"ODE sampler: {nstates} accepted states exceed the trajectory capacity {self.TRAJ_CAP}")
        dscale = (1 - eps) / (1000 if num_steps is None else num_steps)
        self._phase(5, traj, dscale=dscale, do_denoise=1 if denoise else 0, nstates=nstates)
        for s_ in sts:
            s_["nfev"] = int(s_["nfev"]) + (1 if denoise else 0)
        self.last_stats = st
        xs = None
        if traj is not None:
            xs = traj[:nstates].reshape(nstates, self.R, 9).permute(1, 0, 2).clone()
        return xs, self.x_out[: nb_in * self.K].clone()
