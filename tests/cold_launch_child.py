"""Child process of test_gpu_cold_launch.py: in a process that has launched nothing yet, one call of every step entry point whose kernels
need the dynamic-LDS attribute, under every plan it accepts (chain plan first, then 64 / 32 / 16-row tiles, then the head-split plan), each
as the process's first use of that kernel.  Per call: GP_OK, a clean synchronise, finite buffers, and a second identical call (every buffer
put back first) that leaves the same bits.  Stops at the first failure and launches nothing more; prints one JSON line."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from genpose_amd import _lib, samplers
from genpose_amd._lib import ptr, stream_ptr
from genpose_amd.scorenet import ScoreNetHIP
from genpose_amd.weights_synth import make_state_dict

HS = _lib.PLAN_HEADSPLIT
N = 2  # steps of every schedule
done = []


def fail(what):
    print(json.dumps({"ok": False, "failed": what, "calls": done}))
    sys.exit(1)


def twice(name, call, bufs):
    """call() -> return code, twice from the same buffer contents."""
    before = [b.clone() for b in bufs]
    after = []
    for rep in range(2):
        for b, b0 in zip(bufs, before):
            b.copy_(b0)
        rc = call()
        if rc != 0:
            fail(f"{name}: call {rep} returned {rc}")
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            fail(f"{name}: synchronise after call {rep}: {e}")
        after.append([b.clone() for b in bufs])
    for i, (u, v) in enumerate(zip(*after)):
        if not bool(torch.isfinite(u).all()):
            fail(f"{name}: buffer {i} is not finite")
        if not torch.equal(u, v):
            fail(f"{name}: buffer {i} differs between two identical calls")
    done.append(name)


def main():
    dev = torch.device("cuda")
    L = _lib.lib()
    score_net = ScoreNetHIP(make_state_dict(0, "score"), dev)
    energy_net = ScoreNetHIP(make_state_dict(0, "energy"), dev)
    x9 = [ptr(w) for w in score_net.w.bf16x9_packs()]
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    zeros = lambda *s, **kw: torch.zeros(*s, device=dev, **kw)
    feat = rnd(1, 1024).abs()  # one cloud
    cvec, cvec_e = score_net.cloud_embed(feat), energy_net.cloud_embed(feat)
    centre = rnd(1, 3) * 0.3
    sigma = torch.full((1,), 0.7, device=dev)
    st = stream_ptr()

    def table(times, sched, net=score_net):
        return net.time_embed(torch.as_tensor(times, dtype=torch.float32).to(dev)), torch.as_tensor(sched).float().contiguous().to(dev)

    pc_tvec, pc_sched = table(*samplers.pc_schedule(N))
    pc_tvec_e, _ = table(*samplers.pc_schedule(N), net=energy_net)
    heun_tvec, heun_sched = table(*samplers.heun_schedule(N))
    dpm_tvec, dpm_sched = table(*samplers.dpm2m_schedule(N))
    lik_tvec, lik_sched = table(*samplers.heun_likelihood_schedule(N))
    seed_state = torch.tensor([1234, 0, 0, 0], dtype=torch.int64, device=dev)

    def rows(plan):  # one full workgroup and a ragged one
        return (plan & ~HS) + 1

    # ---- score evaluation
    for plan in (128, 64, 32, 16):
        K = rows(plan)
        x, out = rnd(K, 9), zeros(K, 9)
        twice(f"gp_score_eval_plan[{plan}]",
              lambda: L.gp_score_eval_plan(plan, 1, K, score_net.w.ref(), ptr(cvec), ptr(pc_tvec[0]), ptr(x), ptr(sigma), 0, ptr(out), st), [x, out])

    # ---- PC step (launch 0: the first evaluation), score and energy model, then seeded
    def pc(name, entry, model, plan, net, seeded=False, packs=()):
        K = rows(plan)
        t_out, n_out = ctypes.c_int(0), ctypes.c_int(0)
        if L.gp_pc_layout(model, plan, 1, 1, K, ctypes.byref(t_out), ctypes.byref(n_out)) != 0 or t_out.value != plan:
            fail(f"gp_pc_layout({model}, {plan}, 1, 1, {K})")
        x, mean_x, score, partials = rnd(K, 9), zeros(K, 9), zeros(K, 9), zeros(N, n_out.value)
        z1, z2 = rnd(N, K, 9), rnd(N, K, 9)
        noise = (ptr(seed_state),) if seeded else (ptr(z1), ptr(z2))
        head = () if packs else ((plan,) if seeded else (model, plan))
        cv, tvec = (cvec, pc_tvec) if net is score_net else (cvec_e, pc_tvec_e)
        twice(name, lambda: getattr(L, entry)(*head, 1, 1, K, 0, N, net.w.ref(), ptr(cv), ptr(tvec), ptr(pc_sched), *noise, ptr(centre), ptr(x),
                                              ptr(mean_x), ptr(score), ptr(partials), None, None, 0, *packs, st), [x, mean_x, score, partials])

    for plan in (128, 64, 32, 16, 16 | HS):
        pc(f"gp_pc_step_plan[score, {plan}]", "gp_pc_step_plan", 0, plan, score_net)
    for plan in (128, 16):
        pc(f"gp_pc_step_plan[energy, {plan}]", "gp_pc_step_plan", 1, plan, energy_net)
    for plan in (128, 64, 32, 16, 16 | HS):
        pc(f"gp_pc_step_plan_seeded[{plan}]", "gp_pc_step_plan_seeded", 0, plan, score_net, seeded=True)

    # ---- fixed-step solvers: launch 0 of the chain, then the whole solve in one launch
    def fixed(name, entry, plan, tvec, sched, solve=False, packs=()):
        K = rows(plan)
        x, d, score, out = rnd(K, 9), zeros(K, 9), zeros(K, 9), zeros(K, 9)
        head = () if packs else (plan,)
        launch = () if solve else (0,)
        twice(name, lambda: getattr(L, entry)(*head, 1, 1, K, *launch, N, 1, score_net.w.ref(), ptr(cvec), ptr(tvec), ptr(sched), ptr(centre), ptr(x), ptr(d),
                                              ptr(score), ptr(out), None, *packs, st), [x, d, score, out])

    for solver, tvec, sched in (("heun", heun_tvec, heun_sched), ("dpm2m", dpm_tvec, dpm_sched)):
        for plan in (128, 64, 32, 16):
            fixed(f"gp_{solver}_step_plan[{plan}]", f"gp_{solver}_step_plan", plan, tvec, sched)
        for plan in (64, 32, 16):
            fixed(f"gp_{solver}_solve_tile[{plan}]", f"gp_{solver}_solve_tile", plan, tvec, sched, solve=True)

    # ---- the bf16x9 step entry points (chain plan)
    pc("gp_pc_step_bf16x9", "gp_pc_step_bf16x9", 0, 128, score_net, packs=x9)
    pc("gp_pc_step_bf16x9_seeded", "gp_pc_step_bf16x9_seeded", 0, 128, score_net, seeded=True, packs=x9)
    fixed("gp_heun_step_bf16x9", "gp_heun_step_bf16x9", 128, heun_tvec, heun_sched, packs=x9)
    fixed("gp_dpm2m_step_bf16x9", "gp_dpm2m_step_bf16x9", 128, dpm_tvec, dpm_sched, packs=x9)

    # ---- likelihood: 16-row tiles
    K = rows(16)
    x, d, score, div, z = rnd(K, 9), zeros(K, 10), zeros(K, 9), zeros(K), zeros(K, 9)
    logp = zeros(K, dtype=torch.float64)
    twice("gp_heun_likelihood_step", lambda: L.gp_heun_likelihood_step(1, K, 0, N, score_net.w.ref(), ptr(cvec), ptr(lik_tvec), ptr(lik_sched), ptr(x), ptr(d),
                                                                       ptr(score), ptr(div), ptr(logp), ptr(z), st), [x, d, score, div, logp, z])
    eps, tv, tv_e = rnd(K, 9), ptr(pc_tvec[0]), ptr(pc_tvec_e[0])
    twice("gp_score_div", lambda: L.gp_score_div(1, K, score_net.w.ref(), ptr(cvec), tv, ptr(x), ptr(eps), ptr(sigma), ptr(score), ptr(div), st), [x, score, div])
    twice("gp_energy_score", lambda: L.gp_energy_score(1, K, energy_net.w.ref(), ptr(cvec_e), tv_e, ptr(x), ptr(sigma), ptr(score), ptr(div), st),
          [x, score, div])
    twice("gp_score_div_exact", lambda: L.gp_score_div_exact(1, K, score_net.w.ref(), ptr(cvec), tv, ptr(x), ptr(sigma), ptr(score), ptr(div), st),
          [x, score, div])
    print(json.dumps({"ok": True, "calls": done}))


if __name__ == "__main__":
    main()
