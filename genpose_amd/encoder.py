"""PointNet++(MSG) encoder on the HIP kernels - drop-in for `Pointnet2ClsMSG(0)` (networks/pts_encoder/pointnet2.py:166-211).

forward(pts [B,N,3] f32 on the GPU) -> [B,1024].  Launch sequence per call (all on torch's current stream):
  1 x gp_fps_chain      FPS + gather for every level (one workgroup per cloud)
  L x gp_ball_query_msg both radii of a level in one pass
  then per level, what launch_plan(B) lists:
  1 x gp_point_linear   hoisted feature half of the first layer, once per source point (both scales; not at level 0, which has no features)
  1 x the scale's kernel, per scale: gather -> xyz half of layer 1 -> layers 2-3 -> max-pool
Intermediate features stay point-major [B, n, C]; the reference's grouped [B,C+3,np,ns] tensors never exist.

The kernels of a scale.  The constructor decides once which one serves each (level, scale) - the table `_plan`, reported by `sa_kernels` and
`level3_kernel` - and forward() only looks the entry up.  Earlier rows win; a kernel with a minimum batch gives way to the fp32 kernel
below it, with that kernel's bits:
  name     entry point                asked for by         serves                                       minimum batch
  bf16x3   gp_sa_pre_mlp_max_bf16x3   precision='bf16x3'   grouping levels 1.., BF16X3_SHAPES           -
           OPT-IN, exploratory: layers 2-3 as three-term split products, fp32 accumulation (csrc/sa_bf16x3.hip; ~2^-17 relative per product)
  bf16x9   gp_sa_pre_mlp_max_bf16x9   precision='bf16x9'   grouping level 2, BF16X9_SHAPES              -
           layers 2-3 on the BF16 matrix pipe as exact-product split bf16: every operand hi + mid + lo, all nine products exact, fp32
           accumulation - the fp32 kernels' error class (csrc/sa_bf16x9.hip)
  bf16x9   gp_sa_lds_bf16x9           level1='bf16x9'      grouping level 1, LEVEL1_BF16X9_SHAPES       LEVEL1_BF16X9_MIN_CLOUDS
           the same arithmetic with both layers' weights LDS-resident (csrc/sa_lds_bf16x9.hip)
  bf16x9   gp_sa_groupall_bf16x9      level3='bf16x9'      the light encoder's GroupAll level, whole    LEVEL3_BF16X9_MIN_CLOUDS
           ONE launch for the level: all three layers of both scales in that arithmetic, straight from the level-2 features - no hoisted GEMM,
           no zeroing (csrc/sa_groupall_bf16x9.hip)
  f32mfma  gp_sa_pre_mlp_max_layout   default              everything                                   -
           layers 2-3 on the fp32 matrix pipe (register-chain kernels; the hidden-layer layout the weights were packed for, weights.SAScale).
           GroupAll: whole rounds of 256 clouds on the ring kernel (one cloud per workgroup), the rest on 32-row tiles - the tiles of a cloud
           combine by integer atomic max into a zeroed buffer
The three per-scale split kernels work on whole 32-row units, so they serve a scale only where npoint * nsample is a multiple of 32, and a
bf16x9 kernel only where the folded weights split exactly into three normal bf16 terms (weights.split_bf16x9) - for the GroupAll kernel all
six matrices of the level.  Centres and neighbourhoods are unaffected by any of them.

Points per cloud.  Any N >= the first level's npoint (512 in every shipped configuration) is served; fewer points than level 0 selects
raise GenposeHipError (the reference would read past the cloud).  Only the grouping front end depends on N:
  centres   N <= 1024 and at most three grouping levels: gp_fps_chain (one wave per cloud; a level of exactly 64 * 2^k points takes the
            form without bounds checks).  N > 1024, or four grouping levels ('lighter'): one gp_furthest_point_sampling + torch.gather
            per level - n <= 1024 on one wave, <= 2048 / <= 4096 on four waves with 8 / 16 register-resident points per thread, beyond
            that the running minima in global memory.  prepare_grouping(defer_join=True) splits the levels over two streams only in
            the gp_fps_chain range; elsewhere it is the plain sequence on the calling stream.
  balls     a two-scale level: gp_ball_query_msg while the source cloud fits its LDS (gp_ball_query_msg_fits: n <= 5053 at 16 + 32
            samples, n <= 4989 at 32 + 64), else gp_ball_query once per scale into zeroed rows - the cloud in LDS while 12 n + 16 (nsample
            + 1) bytes fit 60 KiB, candidates from global memory beyond.  A single-scale level always takes the per-scale form.
Levels 1.. see at most 512 source points, so they never leave the small-cloud kernels.  encode() captures whichever sequence applies.
"""
import collections
import ctypes
import itertools
import weakref

import torch

from . import _lib
from ._lib import ptr, stream_ptr
from .config import dist_arith_code
from .graphs import CapturedPasses, capture, pin, unpinned
from .lru import ShapeCache
from .weights import EncoderWeights


_GENERATION = itertools.count(1)  # process-wide: every write of a workspace's grouping buffers gets a generation no other write has


class _Kernel(collections.namedtuple("_Kernel", "name entry operands min_clouds fallback")):
    """One entry of the launch plan.  name: what `sa_kernels` / `level3_kernel` report; entry: the C entry point; operands(): the weight
    operands between bias1 and the output (device tensors, packed on first use); min_clouds: the encoder attribute that holds the smallest
    batch the kernel serves, or None; fallback: the entry that serves smaller batches."""

    def at(self, enc, B):
        # (the threshold is read through the instance at call time: it can be set on one encoder)
        return self.fallback if self.min_clouds is not None and B < getattr(enc, self.min_clouds) else self


class Pointnet2EncoderHIP:
    def __init__(self, state_dict, device="cuda", params="light", prefix="pts_encoder.", arith=None, precision="f32", level3=None, level1=None):
        """arith: contraction convention of the squared distances in furthest point sampling and the ball queries ('A' | 'B' | 'C',
        config.DEFAULT_DIST_ARITH when None; include/genpose_hip.h GP_ARITH_*).
        precision ('f32' | 'bf16x9' | 'bf16x3'), level1 and level3 (None / 'f32mfma' | 'bf16x9') ask for the split-bf16 kernels of the
        module text's table; the defaults of this class are the fp32 kernels throughout, an agent's come from config.encoder_kwargs_of
        (a PC-sampler agent asks for all three bf16x9 kernels)."""
        if precision not in ("f32", "bf16x3", "bf16x9"):
            raise ValueError(f"encoder precision {precision!r}: 'f32', 'bf16x9' or 'bf16x3'")
        if level3 not in (None, "f32mfma", "bf16x9"):
            raise ValueError(f"encoder level3 {level3!r}: 'f32mfma' or 'bf16x9'")
        if level1 not in (None, "f32mfma", "bf16x9"):
            raise ValueError(f"encoder level1 {level1!r}: 'f32mfma' or 'bf16x9'")
        self.precision = precision
        self.level1 = level1 or "f32mfma"
        self.level3 = level3 or "f32mfma"
        self.device = torch.device(device)
        self.arith = dist_arith_code(arith)
        self.w = EncoderWeights(state_dict, self.device, params, prefix)
        self.cfg = self.w.cfg
        self.out_dim = self.w.out_dim
        # workspaces (~1.5 MB per cloud) per (batch, points, slot): least recently used first, except those a captured graph writes
        # into (`_pins`: taken by whoever captures, given back when that graph is dropped)
        self._ws = ShapeCache(self.MAX_WORKSPACES, can_evict=unpinned)
        self._pass_graphs = CapturedPasses(self.MAX_PASS_GRAPHS)
        # The launch plan: _plan[k][i] serves scale i of level k, _groupall the GroupAll level as a whole (its fp32 fallback = that level's
        # _plan row behind gp_point_linear).  Rows in order of precedence, as in the module text.  All three per-scale split kernels need
        # whole 32-row units, (B * npoint * nsample) % 32 == 0: decided here for any B as (npoint * nsample) % 32 == 0, which holds for
        # every shape of the three tables under the light, dense and lighter configurations (every npoint is a multiple of 32).
        self._plan = []
        for k, npnt in enumerate(self.cfg["npoints"]):
            row = []
            for sc, ns in zip(self.w.levels[k], self.cfg["nsamples"][k]):
                fp32 = _Kernel("f32mfma", "gp_sa_pre_mlp_max_layout", lambda sc=sc: sc.layers[1] + sc.layers[2], None, None)  # (w2, b2, w3, b3)
                shape = (tuple(sc.couts), ns)
                kern = fp32
                if k > 0 and npnt is not None and (npnt * ns) % 32 == 0:
                    if precision == "bf16x3" and shape in self.BF16X3_SHAPES:
                        kern = _Kernel("bf16x3", "gp_sa_pre_mlp_max_bf16x3", sc.bf16x3_packs, None, None)
                    elif precision == "bf16x9" and shape in self.BF16X9_SHAPES and sc.bf16x9_packs() is not None:
                        kern = _Kernel("bf16x9", "gp_sa_pre_mlp_max_bf16x9", sc.bf16x9_packs, None, None)
                    elif self.level1 == "bf16x9" and shape in self.LEVEL1_BF16X9_SHAPES and sc.bf16x9_lds_packs() is not None:
                        kern = _Kernel("bf16x9", "gp_sa_lds_bf16x9", sc.bf16x9_lds_packs, "LEVEL1_BF16X9_MIN_CLOUDS", fp32)
                row.append(kern)
            self._plan.append(row)
        self._groupall = None
        if self.level3 == "bf16x9" and self.w.groupall_bf16x9_packs() is not None:
            self._groupall = _Kernel("bf16x9", "gp_sa_groupall_bf16x9", self.w.groupall_bf16x9_packs, "LEVEL3_BF16X9_MIN_CLOUDS", tuple(self._plan[-1]))
        # which kernel serves each (level, scale) of the grouping levels, and the GroupAll level: 'f32mfma' | 'bf16x9' | 'bf16x3'
        self.sa_kernels = {(k, i): kern.name for k, row in enumerate(self._plan) if self.cfg["npoints"][k] is not None for i, kern in enumerate(row)}
        self.level3_kernel = self._groupall.name if self._groupall is not None else "f32mfma"

    MAX_WORKSPACES = 12
    # batches from this many clouds up take the split-bf16 GroupAll kernel under level3 = 'bf16x9' (one 128-row item per CU and scale:
    # below, the fp32 tile kernels split finer; measured crossover, profiles/sa_groupall_bf16x9.txt)
    LEVEL3_BF16X9_MIN_CLOUDS = 128
    # batches from this many clouds up take the LDS-resident split-bf16 kernel under level1 = 'bf16x9': the smallest measured size at which
    # both scales together win against the fp32 kernels (profiles/sa_lds_bf16x9.txt: at 5 clouds one 12-wave workgroup copies 72 KB of
    # weights for a handful of units and the pair ties); below, the fp32 kernels with their bits
    LEVEL1_BF16X9_MIN_CLOUDS = 64
    # (layer widths, neighbourhood size) the LDS-resident exact-product split-bf16 kernel is instantiated for: grouping level 1 of the
    # light / dense encoders (csrc/sa_lds_bf16x9.hip)
    LEVEL1_BF16X9_SHAPES = {((64, 64, 128), 16), ((64, 96, 128), 32)}
    # (layer widths, neighbourhood size) the exact-product split-bf16 kernel is instantiated for: grouping level 2 (csrc/sa_bf16x9.hip)
    BF16X9_SHAPES = {((128, 196, 256), 16), ((128, 196, 256), 32)}
    # (layer widths, neighbourhood size) the opt-in split-bf16 kernel is instantiated for: grouping levels 1 and 2 (csrc/sa_bf16x3.hip)
    BF16X3_SHAPES = {((128, 196, 256), 16), ((128, 196, 256), 32), ((64, 64, 128), 16), ((64, 96, 128), 32), ((64, 64, 128), 32)}

    def pin_workspaces(self, B, N, slot=0):
        """For whoever CAPTURES launches of this encoder in a hipGraph: the workspace of that geometry stays out of the eviction order
        while the graph lives (its buffers were allocated outside the capture; nothing but this cache holds them).  Returns the
        workspace; graphs.capture(pins=) takes the pin this way and graphs.release gives it back when the graph is dropped."""
        return pin(self._workspace(B, N, slot))

    def _wait_pending_join(self, ws):
        """A deferred grouping (prepare_grouping(defer_join=True)) whose consumer never ran - an exception in between, a caller that only
        wanted the ticket - leaves work on the side stream that reads new_xyz[0] and writes the deeper levels: every writer of the
        grouping buffers waits for it first."""
        pending = ws.pop("_join", None)
        if pending:
            for ev in pending.values():  # {level: event}
                torch.cuda.current_stream(self.device).wait_event(ev)

    # ------------------------------------------------------------------ workspace (cached per batch/size)
    def _workspace(self, B, N, slot=0):
        key = (B, N, slot)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        dev = self.device
        ws = {"fps_idx": [], "new_xyz": [], "bq": [], "feat": [], "z": []}
        n = N
        cin = 0
        for k, npnt in enumerate(self.cfg["npoints"]):
            cout = sum(s.couts[-1] for s in self.w.levels[k])
            if npnt is None:
                ws["feat"].append(torch.zeros(B, 1, cout, device=dev))
                ws["z"].append(torch.empty(B, n, sum(s.couts[0] for s in self.w.levels[k]), device=dev) if cin > 0 else None)
                break
            ws["fps_idx"].append(torch.empty(B, npnt, dtype=torch.int32, device=dev))
            ws["new_xyz"].append(torch.empty(B, npnt, 3, device=dev))
            ws["bq"].append([torch.empty(B, npnt, ns, dtype=torch.int32, device=dev) for ns in self.cfg["nsamples"][k]])
            ws["feat"].append(torch.empty(B, npnt, cout, device=dev))
            zs = sum(s.couts[0] for s in self.w.levels[k])
            ws["z"].append(torch.empty(B, n, zs, device=dev) if cin > 0 else None)
            n, cin = npnt, cout
        self._ws[key] = ws
        return ws

    def sample_centres(self, pts, slot=0):
        """Stage 1 of forward(): furthest point sampling + gather for every level into workspace `slot` (launches on the
        current stream).  Latency-bound and light (one workgroup per cloud), so a pipeline can run it for the NEXT batch on a
        side stream while the MFMA-heavy stages of the current one own the chip; forward(..., slot=slot, centres_done=True)
        then skips it."""
        _lib.check_device()
        if not pts.is_cuda or pts.dtype != torch.float32:
            raise RuntimeError("pts must be a float32 CUDA tensor")
        xyz0 = pts[..., 0:3].contiguous()
        B, N, _ = xyz0.shape
        ws = self._workspace(B, N, slot)
        self._wait_pending_join(ws)
        ws["_gen"] = next(_GENERATION)  # fps_idx / new_xyz are about to be overwritten: tickets for the previous contents die here
        st = stream_ptr()
        cfg = self.cfg
        group_levels = [k for k, npnt in enumerate(cfg["npoints"]) if npnt is not None]
        if len(group_levels) <= 3 and N <= 1024:
            m = (ctypes.c_int * 3)(*([cfg["npoints"][k] for k in group_levels] + [0] * (3 - len(group_levels))))
            pi = [ptr(ws["fps_idx"][l]) if l < len(group_levels) else None for l in range(3)]
            px = [ptr(ws["new_xyz"][l]) if l < len(group_levels) else None for l in range(3)]
            _lib.call("gp_fps_chain_arith", self.arith, B, N, len(group_levels), m, ptr(xyz0), pi[0], px[0], pi[1], px[1], pi[2], px[2], st)
        else:
            cur = xyz0
            for l, k in enumerate(group_levels):
                npnt = cfg["npoints"][k]
                temp = torch.full((B, cur.shape[1]), 1e10, device=self.device)
                _lib.call("gp_furthest_point_sampling_arith", self.arith, B, cur.shape[1], npnt, ptr(cur), ptr(temp), ptr(ws["fps_idx"][l]), st)
                torch.gather(cur, 1, ws["fps_idx"][l].long().unsqueeze(-1).expand(B, npnt, 3), out=ws["new_xyz"][l])
                cur = ws["new_xyz"][l]
        return xyz0

    def _ball_queries(self, ws, xyz0, B, N, levels=None):
        """Ball queries of every grouping level (they depend on the coordinates only) into ws['bq']; `levels`: only those levels."""
        if levels is None:  # (a level-restricted call is prepare_grouping's own, which has just handled the pending join)
            self._wait_pending_join(ws)
        ws["_gen"] = next(_GENERATION)  # every writer of the grouping buffers invalidates outstanding tickets
        st = stream_ptr()
        cfg = self.cfg
        xyz, n = xyz0, N
        for k, npnt in enumerate(cfg["npoints"]):
            if npnt is None:
                break
            new_xyz = ws["new_xyz"][k]
            if levels is not None and k not in levels:
                xyz, n = new_xyz, npnt
                continue
            radii, nss = cfg["radii"][k], cfg["nsamples"][k]
            # two scales in one pass while the cloud fits the fused kernel's LDS (n <= 5053 at 16 + 32 samples: the C side owns the limit);
            # a larger cloud, like a level of one or three scales: one query per scale into zeroed rows, which takes any n
            if len(self.w.levels[k]) == 2 and _lib.lib().gp_ball_query_msg_fits(n, nss[0], nss[1]):
                _lib.call("gp_ball_query_msg_arith", self.arith, B, n, npnt, float(radii[0]), nss[0], float(radii[1]), nss[1], ptr(new_xyz), ptr(xyz),
                          ptr(ws["bq"][k][0]), ptr(ws["bq"][k][1]), st)
            else:
                for i in range(len(self.w.levels[k])):
                    ws["bq"][k][i].zero_()
                    _lib.call("gp_ball_query_arith", self.arith, B, n, npnt, float(radii[i]), nss[i], ptr(new_xyz), ptr(xyz), ptr(ws["bq"][k][i]), st)
            xyz, n = new_xyz, npnt

    def grouping_key(self):
        """Everything the sampled centres and neighbourhoods depend on besides the coordinates."""
        c = self.cfg
        return (tuple(c["npoints"]), tuple(map(tuple, c["radii"])), tuple(map(tuple, c["nsamples"])), self.arith)

    def prepare_grouping(self, pts, slot=0, defer_join=False):
        """Furthest point sampling + gather + ball queries for every level into workspace `slot`; returns that workspace.  These
        depend on the point coordinates only - not on any weight - so a second encoder with the same grouping configuration (the
        energy model's, which sees the same clouds) can take them over: forward(pts, grouping=<this workspace>).

        defer_join (the encoder pass of an agent call): furthest point sampling is a chain of dependent block-wide argmax steps - 57 % of
        them belong to level 0 - that occupies one wave per SIMD and no matrix pipe.  Only level 0 is sampled on the calling stream;
        the deeper levels and their ball queries go to a side stream and run UNDERNEATH the level-0 set abstraction (ball query, both
        chain kernels, the hoisted GEMM of level 1).  The workspace then carries the join event (`_join`), which forward(grouping=ws)
        waits for before its first use of a deeper level."""
        self._wait_pending_join(self._workspace(pts.shape[0], pts.shape[1], slot))  # a deferred grouping nobody consumed
        cfg = self.cfg
        group_levels = [k for k, npnt in enumerate(cfg["npoints"]) if npnt is not None]
        if not (defer_join and 2 <= len(group_levels) <= 3 and pts.shape[1] <= 1024 and pts.is_cuda):
            xyz0 = self.sample_centres(pts, slot)
            B, N, _ = xyz0.shape
            ws = self._workspace(B, N, slot)
            self._ball_queries(ws, xyz0, B, N)
            ws["_grouping_key"] = self.grouping_key()
            return ws
        _lib.check_device()
        if pts.dtype != torch.float32:
            raise RuntimeError("pts must be a float32 CUDA tensor")
        xyz0 = pts[..., 0:3].contiguous()
        B, N, _ = xyz0.shape
        ws = self._workspace(B, N, slot)
        ws["_gen"] = next(_GENERATION)
        cur = torch.cuda.current_stream(self.device)
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(self.device)
        m0 = (ctypes.c_int * 3)(cfg["npoints"][group_levels[0]], 0, 0)
        _lib.call("gp_fps_chain_arith", self.arith, B, N, 1, m0, ptr(xyz0), ptr(ws["fps_idx"][0]), ptr(ws["new_xyz"][0]), None, None, None, None, stream_ptr())
        fork = torch.cuda.Event()
        fork.record(cur)
        joins = {}
        with torch.cuda.stream(self._side):
            self._side.wait_event(fork)
            # the deeper levels select among the previous level's centres, in their order (the reference samples new_xyz of the level
            # before): ONE level per launch, each followed by its ball query and its own join event, so that the set abstraction of level k
            # starts as soon as ITS centres and neighbourhoods exist - level 1's kernels run beside level 2's sampling (round 6: at 5 clouds
            # the fused two-level chain held the pass for 97 us of sampling + both ball queries; a level at a time it is 60 us + one)
            n_src = cfg["npoints"][group_levels[0]]
            for l, k in enumerate(group_levels[1:]):
                mk = (ctypes.c_int * 3)(cfg["npoints"][k], 0, 0)
                _lib.call("gp_fps_chain_arith", self.arith, B, n_src, 1, mk, ptr(ws["new_xyz"][l]), ptr(ws["fps_idx"][l + 1]), ptr(ws["new_xyz"][l + 1]), None, None,
                          None, None, stream_ptr())
                self._ball_queries(ws, xyz0, B, N, levels={k})
                joins[k] = torch.cuda.Event()
                joins[k].record(self._side)
                n_src = cfg["npoints"][k]
        self._ball_queries(ws, xyz0, B, N, levels={group_levels[0]})
        ws["_join"] = joins  # {level: event}
        ws["_grouping_key"] = self.grouping_key()
        return ws

    def grouping_ticket(self, pts, ws):
        """What a second encoder needs to take this grouping over safely (GFObjectPose.extract_pts_feature): WHICH tensor object the
        clouds are (a weak reference - an address can be reused by the allocator, an object cannot), which version of it (in-place
        edits bump `_version`), and which generation of the workspace (every writer of the grouping buffers - prepare_grouping, a plain
        forward(), sample_centres - takes a fresh process-wide generation, so a ticket never outlives the contents it was issued for)."""
        return {"ws": ws, "gen": ws["_gen"], "key": self.grouping_key(), "pts": weakref.ref(pts), "version": pts._version, "shape": tuple(pts.shape)}

    @staticmethod
    def ticket_valid(ticket, pts, key):
        return (ticket is not None and ticket["key"] == key and ticket["pts"]() is pts and ticket["version"] == pts._version
                and ticket["shape"] == tuple(pts.shape) and ticket["ws"].get("_gen") == ticket["gen"])

    MAX_PASS_GRAPHS = 8  # captured encoder passes kept per encoder (least recently used first)

    def encode(self, pts, grouping=None, use_graph=True):
        """The whole encoder pass of an AGENT call (GFObjectPose.extract_pts_feature) as one hipGraph replay per input shape:
            grouping None  ->  prepare_grouping + forward: returns (feat [B,1024], workspace) - the workspace is what a second encoder takes
                               over (grouping_ticket);
            grouping = ws  ->  forward on those centres and neighbourhoods: returns feat.
        ~25 launches replayed instead of issued (they dominate a small batch: a 5-cloud pass is launch-bound).  The first call of a shape
        runs launch by launch (warm-up; a shape seen once never pays a capture), the second captures, later ones copy the clouds into the
        graph's static input and replay.  Results are the launch-by-launch pass's, bit for bit (same kernels, same order)."""
        run = (lambda p: self.forward(p, grouping=grouping)) if grouping is not None else self._forward_with_grouping
        if not use_graph or not pts.is_cuda or pts.dtype != torch.float32 or torch.cuda.is_current_stream_capturing():
            return run(pts)  # (wrong device / dtype: the launch-by-launch path raises what it always raised)

        def captured():
            buf = pts[..., 0:3].contiguous().clone()
            # (no warm-up: the first call of the shape was one; `grouping` is kept alive - its id() is part of the key)
            return capture(lambda: run(buf), bufs=(buf,), pins=[lambda: self.pin_workspaces(buf.shape[0], buf.shape[1], 0)],
                           extra={"grouping": grouping})
        # (the id() of `grouping` is part of the key: an entry with a graph keeps its `grouping` alive, so the id cannot be reused
        # while the entry lives; a shape only SEEN so far is remembered by shape alone)
        key = (tuple(pts.shape), id(grouping) if grouping is not None else None)
        ent = self._pass_graphs.entry(key, (tuple(pts.shape), grouping is not None), captured)
        if ent is None:
            return run(pts)
        if grouping is not None:
            return ent.replay(pts[..., 0:3]).clone()
        ent.outs[1]["_gen"] = next(_GENERATION)  # the replay rewrites the grouping buffers: tickets for the previous contents die here
        feat, ws = ent.replay(pts[..., 0:3])
        return feat.clone(), ws

    def _forward_with_grouping(self, pts):
        ws = self.prepare_grouping(pts, defer_join=True)
        return self.forward(pts, grouping=ws), ws

    def _whole_level(self, k, B):
        """The kernel that serves all of level k in one launch for B clouds, or None: gp_point_linear + one kernel per scale."""
        if self.cfg["npoints"][k] is None and self._groupall is not None and self._groupall.at(self, B) is self._groupall:
            return self._groupall
        return None

    def launch_plan(self, B):
        """The C entry points the set-abstraction levels of a pass over B clouds call, in launch order (what forward() issues after the
        grouping front end, whose launches depend on N: module text).  Pure host logic: no device is touched."""
        names = []
        for k, row in enumerate(self._plan):
            whole = self._whole_level(k, B)
            if whole is not None:
                names.append(whole.entry)
                continue
            if k > 0:  # (a level behind another has input features, and with them the hoisted half of layer 1: _workspace's `z`)
                names.append("gp_point_linear")
            names += [kern.at(self, B).entry for kern in row]
        return names

    def forward(self, pts, return_intermediates=False, slot=0, centres_done=False, grouping=None):
        """grouping: workspace returned by prepare_grouping() of an encoder with the same grouping configuration, for the SAME
        clouds: its centres and neighbourhood indices are used instead of being recomputed."""
        _lib.check_device()
        if not pts.is_cuda or pts.dtype != torch.float32:
            raise RuntimeError("pts must be a float32 CUDA tensor")
        xyz0 = pts[..., 0:3].contiguous()
        B, N, _ = xyz0.shape
        ws = self._workspace(B, N, slot)
        st = stream_ptr()
        cfg = self.cfg
        if grouping is not None:
            if grouping.get("_grouping_key") != self.grouping_key() or grouping["new_xyz"][0].shape[0] != B:
                raise ValueError("grouping comes from an encoder with a different configuration / batch")
            src = grouping
        else:
            src = ws
            if not centres_done:
                self._wait_pending_join(ws)
            # ---- furthest point sampling + gather for every level
            if not centres_done:
                self.sample_centres(pts, slot)
            self._ball_queries(ws, xyz0, B, N)
        # ---- set abstraction levels: the launches launch_plan(B) lists
        xyz, feats, n, cin = xyz0, None, N, 0
        for k, npnt in enumerate(cfg["npoints"]):
            scales = self.w.levels[k]
            out = ws["feat"][k]
            cout_total = out.shape[-1]
            if self._whole_level(k, B) is not None:
                # GroupAll in one launch, straight from the level-2 features: every output column written whole (no hoisted rows, no zeroing)
                wx9, offs = self._groupall.operands()
                sargs = []
                for i, sc in enumerate(scales):
                    (_, b1), (_, b2), (_, b3) = sc.layers
                    sargs += [sc.couts[1], ptr(wx9[offs[i]:]), ptr(sc.wxyz), ptr(b1), ptr(b2), ptr(b3), i * sc.couts[2]]
                _lib.call(self._groupall.entry, B, n, cin, scales[0].couts[0], scales[0].couts[2], ptr(xyz), ptr(feats), *sargs, ptr(out), cout_total, st)
                xyz, feats, n, cin = None, out, 1, cout_total
                continue
            if npnt is None:
                # GroupAll is one neighbourhood of all n points around no centre; the tiles of a cloud combine through an integer atomic
                # max into the zeroed output
                out.zero_()
                new_xyz, npnt, nss, idx = None, 1, [n] * len(scales), [None] * len(scales)
            else:
                new_xyz, nss, idx = src["new_xyz"][k], cfg["nsamples"][k], src["bq"][k]
            # first layer hoisted: feature half once per source point, xyz half while gathering (csrc/sa_mlp.hip)
            z = ws["z"][k]
            zstride = sum(sc.couts[0] for sc in scales)
            if z is not None:
                _lib.call("gp_point_linear", B * n, cin, zstride, ptr(feats), ptr(self.w.z_weights[k]), ptr(z), st)
            if k >= 1 and src.get("_join") and k in src["_join"]:
                # deferred grouping (prepare_grouping(defer_join=True)): this level's centres and neighbourhoods were computed on the
                # side stream under the levels before it - first use here
                torch.cuda.current_stream(self.device).wait_event(src["_join"].pop(k))
                if not src["_join"]:
                    src.pop("_join")
            off, zoff = 0, 0
            for i, sc in enumerate(scales):
                kern = self._plan[k][i].at(self, B)
                lead = (sc.hidden_layout,) if kern.entry == "gp_sa_pre_mlp_max_layout" else ()
                _lib.call(kern.entry, *lead, B, n, npnt, nss[i], sc.couts[0], sc.couts[1], sc.couts[2], ptr(xyz), ptr(new_xyz), ptr(idx[i]), ptr(z), zstride, zoff,
                          ptr(sc.wxyz), ptr(sc.layers[0][1]), *map(ptr, kern.operands()), ptr(out), cout_total, off, st)
                off += sc.couts[2]
                zoff += sc.couts[0]
            xyz, feats, n, cin = new_xyz, out, npnt, cout_total
        res = feats.reshape(B, -1).clone()
        if return_intermediates:
            if src is not ws:
                ws = dict(ws, new_xyz=src["new_xyz"], fps_idx=src["fps_idx"], bq=src["bq"])
            return res, ws
        return res

    __call__ = forward
