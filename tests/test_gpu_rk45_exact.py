"""The device RK45 solver (csrc/rk45.hip) against float64 ground truth (tests/rk45_reference.py): single evaluations of analytic-field
networks against their closed form, every logged attempt of a device solve replayed in float64 from the device's own state and step,
the stage derivatives of an attempt against the field at the stage states, whole solves against the exact solution and against
scipy.integrate.RK45's schedule - and the energy ranking on non-finite energies."""
import math

import numpy as np
import pytest
import torch

import rk45_reference as rr
from oracle import genpose_oracle as go

pytestmark = pytest.mark.gpu

PLANS = [16, 32, 64, 128, 16 | 0x100, 16 | 0x200, 48 | 0x200]  # tiles, head-split, shared-chunk (genpose_amd/_lib.py PLAN_*)


def _net(name):
    from genpose_amd.scorenet import ScoreNetHIP
    anet, model = rr.problems()[name]
    return anet, model, ScoreNetHIP(anet.state_dict(go.make_state_dict(0, "score")), "cuda")


def _refusal(model, plan, groups, bpg, K):
    """why the driver refuses (model, plan) at this shape, or None: gp_rk45_partials_count, and the Python-side rule of ODESampler
    (the energy and likelihood models run their backward pass on 16-row tiles or the 128-row chain only)"""
    from genpose_amd import _lib
    from genpose_amd.samplers import ODESampler
    if _lib.lib().gp_rk45_partials_count(ODESampler.MODELS[model], plan, groups, bpg, K) <= 0:
        return "gp_rk45_partials_count refuses the shape"
    tile = plan & ~_lib.PLAN_FLAGS
    if model != "score" and (tile in (32, 48, 64) or plan & _lib.PLAN_HEADSPLIT):
        return "backward-pass models run on 16-row tiles or the 128-row chain"
    return None


# every (model, plan, clouds x candidates, groups) the tests below skip, and why: asserted, not just printed
EXPECTED_SKIPS = {
    ("score", 16 | 0x200, 4, 50, 1): "gp_rk45_partials_count refuses the shape",
    ("score", 48 | 0x200, 4, 50, 1): "gp_rk45_partials_count refuses the shape",
    ("score", 16 | 0x200, 256, 50, 1): "gp_rk45_partials_count refuses the shape",
    ("score", 16 | 0x200, 6, 64, 3): "gp_rk45_partials_count refuses the shape",
    ("score", 48 | 0x200, 6, 64, 3): "gp_rk45_partials_count refuses the shape",
}
for _m in ("energy", "likelihood"):
    EXPECTED_SKIPS.update({(_m, p, 4, 50, 1): "backward-pass models run on 16-row tiles or the 128-row chain" for p in (32, 64, 16 | 0x100)})
    EXPECTED_SKIPS.update({(_m, p, 4, 50, 1): "gp_rk45_partials_count refuses the shape" for p in (16 | 0x200, 48 | 0x200)})


def _sampler(snet, model, B, K, plan, groups=1, **kw):
    from genpose_amd.samplers import ODESampler
    why = _refusal(model, plan, groups, B // groups, K)
    key = (model, plan, B, K, groups)
    assert EXPECTED_SKIPS.get(key) == why, f"plan {plan:#x} for {key}: refused because {why!r}, expected {EXPECTED_SKIPS.get(key)!r}"
    if why is not None:
        return None
    return ODESampler(snet, B, K, "cuda", model=model, tile=plan, groups=groups, **kw)


def _problem(anet, snet, model, B, K, T0, seed=0):
    lik = model == "likelihood"
    pf, x, probe = rr.inputs(B, K, T0, seed=seed, likelihood=lik)
    cvec = snet.cloud_embed(torch.from_numpy(pf).cuda())
    c_rows = np.repeat(anet.offsets(pf), K, 0)
    fld = rr.Field(anet, model, c_rows, probe if lik else None)
    Y0 = np.concatenate([x, np.zeros((B * K, 1))], 1) if lik else x.astype(np.float64)
    return cvec, x, probe, c_rows, fld, Y0


# ----------------------------------------------------------------------------- (a) single evaluations against the closed form
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 33, 127, 129, 5141, 12800])
def test_single_evaluations_closed_form(rows):
    anet, _, snet = _net("time")
    K = 50 if rows == 12800 else 1  # one cloud (and one offset) per row, or 256 clouds x 50 candidates
    B = rows // K
    gen = np.random.default_rng(rows)
    pf = np.abs(gen.standard_normal((B, 1024))).astype(np.float32)
    x = (gen.standard_normal((rows, 9)) * 5).astype(np.float32)
    eps = gen.standard_normal((rows, 9)).astype(np.float32)
    c = np.repeat(anet.offsets(pf), K, 0)
    cvec = snet.cloud_embed(torch.from_numpy(pf).cuda())
    xd, epsd = torch.from_numpy(x).cuda(), torch.from_numpy(eps).cuda()
    x64 = x.astype(np.float64)
    for t in (1e-5, 0.3, 1.0):
        tvec = snet.time_embed(torch.tensor([t], device="cuda"))
        sig32 = torch.tensor([0.01 * 5000.0 ** t], device="cuda")
        sig = float(sig32.item())
        f = anet.f_theta(t, x64, c)
        m = anet.magnitude(t, x64, c)
        tol = 32 * rr.U32 * m / sig + 1e-30
        for plan in (0, 16, 64):
            got = snet.evaluate(cvec, K, xd, tvec[0], sig32, "score", tile=plan).cpu().numpy()
            ref = f / (sig + 1e-7)
            assert np.all(np.abs(got - ref) <= tol), (t, plan, np.max(np.abs(got - ref) / tol))
            e = snet.evaluate(cvec, K, xd, tvec[0], sig32, "energy", tile=plan).cpu().numpy()
            e_ref = np.stack([np.sum(x64[:, :6] * f[:, :6], 1), np.sum(x64[:, 6:] * f[:, 6:], 1)], 1) / sig
            e_tol = np.stack([np.sum(np.abs(x64[:, :6]) * m[:, :6], 1), np.sum(np.abs(x64[:, 6:]) * m[:, 6:], 1)], 1) * 32 * rr.U32 / sig
            assert np.all(np.abs(e - e_ref) <= e_tol), (t, plan)
        g = snet.energy_score(cvec, K, xd, tvec[0], sig32).cpu().numpy()
        g_ref = (f + x64 @ anet.A) / sig
        g_tol = 32 * rr.U32 * (m + np.abs(x64) @ np.abs(anet.A)) / sig
        assert np.all(np.abs(g - g_ref) <= g_tol), t
        s, div = (v.cpu().numpy() for v in snet.score_and_divergence(cvec, K, xd, epsd, tvec[0], sig32))
        e64 = eps.astype(np.float64)
        d_ref = np.einsum("ri,ij,rj->r", e64, anet.A, e64) / (sig + 1e-7)
        d_tol = 32 * rr.U32 * np.einsum("ri,ij,rj->r", np.abs(e64), np.abs(anet.A), np.abs(e64)) / sig
        assert np.all(np.abs(s - f / (sig + 1e-7)) <= tol), t
        assert np.all(np.abs(div - d_ref) <= d_tol), t


# ----------------------------------------------------------------------------- (b) + (c) replay and ground truth, every plan
def _same_schedule(run, sc, plan):
    """the device's evaluation count and accept / reject sequence are scipy.integrate.RK45's on the float64 field, attempt for attempt
    (legitimate on the STRICT solves: tests/test_rk45_reference_cpu.py::test_strict_problems_keep_err_norm_away_from_one)"""
    assert int(run["nfev"]) == sc["nfev"], (f"plan {plan:#x}", int(run["nfev"]), sc["nfev"])
    np.testing.assert_array_equal(run["log_acc"].astype(bool), sc["acc"], err_msg=f"plan {plan:#x}")


def _scipy_reference(fld, Y0, t0, t1):
    R = Y0.shape[0]
    return rr.scipy_run(rr.fun_flat(fld, R), t0, Y0.reshape(-1), t1)


# (name, T0, clouds, candidates, strict): strict solves are compared with scipy's whole schedule; the others are path-sensitive
# (tests/test_rk45_reference_cpu.py::test_path_sensitive_problems_are_so) and held to the float64 replay and the exact solution
SCORE_SOLVES = [("contract", 1.0, 4, 50, True), ("contract", 0.55, 4, 50, False), ("contract", 0.15, 4, 50, True), ("time", 1.0, 4, 50, False),
                ("time", 0.55, 4, 50, False), ("contract", 1.0, 256, 50, True)]


@pytest.mark.parametrize("name,T0,B,K,strict", SCORE_SOLVES)
def test_score_solve_replay_and_ground_truth(name, T0, B, K, strict):
    anet, model, snet = _net(name)
    cvec, x, _, c_rows, fld, Y0 = _problem(anet, snet, model, B, K, T0)
    sc = _scipy_reference(fld, Y0, T0, rr.EPS)
    exact = rr.exact_solution(anet, model, Y0, c_rows, T0, [rr.EPS])[0]
    scipy_err = np.abs(sc["states"][-1].reshape(Y0.shape) - exact).max()
    ran = 0
    for plan in PLANS:
        smp = _sampler(snet, model, B, K, plan)
        if smp is None:
            continue
        ran += 1
        run = rr.solve_raw(smp, cvec, torch.from_numpy(Y0).cuda(), T0, rr.EPS)[0]
        worst = rr.replay_check(fld, run, T0, rr.EPS)
        print(f"replay {name} T0={T0} {B}x{K} plan {plan:#x}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        if strict:
            _same_schedule(run, sc, plan)
        # the raw end state is the exact solution to within 4 x scipy's own global error + the float32 floor
        end = run["states"][-1]
        assert np.abs(end - exact).max() <= 4 * scipy_err + 1e-5 * max(1.0, np.abs(exact).max()), plan
        # the production path (denoise, normalize_rotation, centre) from the same start
        centre = torch.randn(B, 3, generator=torch.Generator().manual_seed(1)).cuda()
        _, xout = smp.run(cvec, centre, torch.from_numpy(x).cuda(), T0)
        cen_rows = centre.cpu().double().numpy().repeat(K, 0)
        xd = exact + fld(rr.EPS, exact) * 2.0 * (1 - rr.EPS) / 1000  # denoise: x + (-g^2 score) dscale = x + 2 f_rhs dscale
        ref = torch.from_numpy(xd.copy())
        ref[:, :6] = go.normalize_rotation(ref[:, :6])
        ref[:, 6:] += torch.from_numpy(cen_rows)
        col = np.minimum(np.linalg.norm(xd[:, 0:3], axis=1), np.linalg.norm(xd[:, 3:6], axis=1)).min()
        tol = (4 * scipy_err + 1e-5 * max(1.0, np.abs(exact).max())) * (1 + 4 / col)
        assert np.abs(xout.cpu().numpy() - ref.numpy()).max() <= tol, plan
    assert ran > 0


@pytest.mark.parametrize("num_steps", [2, 20, 1000])
def test_dense_output_exact(num_steps):
    name, T0, B, K = "time", 0.55, 4, 50
    anet, model, snet = _net(name)
    cvec, x, _, c_rows, fld, Y0 = _problem(anet, snet, model, B, K, T0)
    t_eval = np.linspace(T0, rr.EPS, num_steps)
    exact = rr.exact_solution(anet, model, Y0, c_rows, T0, t_eval)
    import scipy.integrate
    sol = scipy.integrate.solve_ivp(rr.fun_flat(fld, B * K), (T0, rr.EPS), Y0.reshape(-1), method="RK45", rtol=1e-5, atol=1e-5, t_eval=t_eval)
    dense_err = np.abs(sol.y.T.reshape(num_steps, B * K, 9) - exact).max()
    centre = torch.zeros(B, 3, device="cuda")
    for plan in PLANS:
        smp = _sampler(snet, model, B, K, plan)
        if smp is None:
            continue
        xs, _ = smp.run(cvec, centre, torch.from_numpy(x).cuda(), T0, num_steps=num_steps, return_process=True)
        xs = xs.cpu().numpy().transpose(1, 0, 2)  # [S, R, 9]
        ref = torch.from_numpy(exact.reshape(-1, 9).copy())
        ref[:, :6] = go.normalize_rotation(ref[:, :6])
        ref = ref.numpy().reshape(num_steps, B * K, 9)
        y0p = torch.from_numpy(Y0.copy())
        y0p[:, :6] = go.normalize_rotation(y0p[:, :6])
        np.testing.assert_allclose(xs[0], y0p.numpy(), rtol=4 * rr.U64, atol=4 * rr.U64)  # the first row is the post-processed y0
        col = min(np.linalg.norm(exact[..., 0:3], axis=-1).min(), np.linalg.norm(exact[..., 3:6], axis=-1).min())
        tol = (4 * dense_err + 1e-5 * max(1.0, np.abs(exact).max())) * (1 + 4 / col)
        assert np.abs(xs - ref).max() <= tol, (plan, np.abs(xs - ref).max(), tol)


@pytest.mark.parametrize("T0", [1.0, 0.55])
def test_energy_model_solve(T0):
    anet, model, snet = _net("energy")
    B, K = 4, 50
    cvec, x, _, c_rows, fld, Y0 = _problem(anet, snet, model, B, K, T0)
    sc = _scipy_reference(fld, Y0, T0, rr.EPS)
    exact = rr.exact_solution(anet, model, Y0, c_rows, T0, [rr.EPS])[0]
    scipy_err = np.abs(sc["states"][-1].reshape(Y0.shape) - exact).max()
    ran = 0
    for plan in PLANS:
        smp = _sampler(snet, model, B, K, plan)
        if smp is None:
            continue
        ran += 1
        run = rr.solve_raw(smp, cvec, torch.from_numpy(Y0).cuda(), T0, rr.EPS)[0]
        worst = rr.replay_check(fld, run, T0, rr.EPS)
        print(f"replay energy T0={T0} plan {plan:#x}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        if T0 == 1.0:  # energy at T0 = 0.55 is path-sensitive
            _same_schedule(run, sc, plan)
        assert np.abs(run["states"][-1] - exact).max() <= 4 * scipy_err + 1e-5 * max(1.0, np.abs(exact).max())
    assert ran > 0


def test_likelihood_solve():
    anet, model, snet = _net("likelihood")
    B, K = 4, 50
    cvec, x, probe, c_rows, fld, Y0 = _problem(anet, snet, model, B, K, rr.EPS)
    z_ex, dlogp_ex, bits_ex = rr.exact_likelihood(anet, x.astype(np.float64), probe.astype(np.float64), c_rows)
    sc = _scipy_reference(fld, Y0, rr.EPS, 1.0)
    end = sc["states"][-1].reshape(Y0.shape)
    err_z, err_l = np.abs(end[:, :9] - z_ex).max(), np.abs(end[:, 9] - dlogp_ex).max()
    from genpose_amd import likelihood
    ran = 0
    for plan in PLANS:
        smp = _sampler(snet, model, B, K, plan)
        if smp is None:
            continue
        ran += 1
        run = rr.solve_raw(smp, cvec, torch.from_numpy(Y0).cuda(), rr.EPS, 1.0, probe=torch.from_numpy(probe).cuda())[0]
        worst = rr.replay_check(fld, run, rr.EPS, 1.0)
        _same_schedule(run, sc, plan)
        print(f"replay likelihood plan {plan:#x}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        z, bits = likelihood.cond_ode_likelihood(snet, cvec, K, torch.from_numpy(x).cuda(), torch.from_numpy(probe).cuda(), solver=smp)
        floor = 1e-5 * max(1.0, np.abs(z_ex).max())
        assert np.abs(z.cpu().numpy() - z_ex).max() <= 4 * err_z + floor, plan
        bits_tol = (4 * err_l + 1e-5 * max(1.0, np.abs(dlogp_ex).max()) + (4 * err_z + floor) * np.abs(z_ex).max() * 2 / rr.SIGMA_MAX ** 2) / math.log(2)
        assert np.abs(bits.cpu().numpy() - bits_ex).max() <= bits_tol, plan
    assert ran > 0


@pytest.mark.parametrize("plan", PLANS)
def test_grouped_solves_replay_per_group(plan):
    """three batches at very different scales share each launch: every group keeps its own schedule and is replayed on its own state"""
    anet, model, snet = _net("time")
    G, B1, K = 3, 2, 64
    T0 = 1.0
    cvec, x, _, c_rows, fld, Y0 = _problem(anet, snet, model, G * B1, K, T0)
    rows = B1 * K
    Y0 = Y0.copy()
    for g, s in enumerate((1.0, 1e-2, 30.0)):
        Y0[g * rows:(g + 1) * rows] *= s
    smp = _sampler(snet, model, G * B1, K, plan, groups=G)
    if smp is None:
        return  # a refusal listed in EXPECTED_SKIPS
    runs = rr.solve_raw(smp, cvec, torch.from_numpy(Y0).cuda(), T0, rr.EPS)
    assert len({int(r["n_attempts"]) for r in runs}) > 1 or len({tuple(r["log_h"][:3]) for r in runs}) > 1, "schedules must differ"
    for g, run in enumerate(runs):
        fg = rr.Field(anet, model, c_rows[g * rows:(g + 1) * rows])
        worst = rr.replay_check(fg, run, T0, rr.EPS)
        print(f"replay grouped plan {plan:#x} group {g}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("tile", [16, 32, 16 | 0x100])
def test_ragged_groups_replay_per_group(tile):
    from genpose_amd.samplers import ODESampler
    anet, model, snet = _net("time")
    K, clouds = 30, [1, 3, 2]
    T0 = 0.55
    B = sum(clouds)
    cvec, x, _, c_rows, fld, Y0 = _problem(anet, snet, model, B, K, T0)
    Y0 = Y0.copy()
    r0 = 0
    for n, s in zip(clouds, (1.0, 1e-2, 20.0)):
        Y0[r0:r0 + n * K] *= s
        r0 += n * K
    smp = ODESampler(snet, 8, K, "cuda", group_clouds=[2, 3, 2, 1], tile=tile)  # capacity; this step's grouping below
    smp.set_groups(clouds)
    runs = rr.solve_raw(smp, cvec, torch.from_numpy(Y0).cuda(), T0, rr.EPS)
    r0 = 0
    for g, (run, n) in enumerate(zip(runs, clouds)):
        fg = rr.Field(anet, model, c_rows[r0:r0 + n * K])
        worst = rr.replay_check(fg, run, T0, rr.EPS)
        print(f"replay ragged tile {tile} group {g}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        r0 += n * K


def _stage_walk(snet, fld, B, K, T0, plan, check):
    """steps one attempt at a time (no graphs) and hands every attempt's (t, h, y, K [7, n], ynew) to check(); returns attempts run"""
    smp = _sampler(snet, "score", B, K, plan, use_graph=False, poll=1)
    if smp is None:
        return 0
    Y0 = fld.Y0
    smp.cvec.copy_(fld.cvec)
    smp.centre.zero_()
    smp.y.copy_(torch.from_numpy(Y0.reshape(-1)).cuda())
    smp._phase(0, None, t0=T0, t_bound=rr.EPS, rtol=1e-5, atol=1e-5)
    smp._phase(1, None)
    smp._phase(2, None)
    for _ in range(200):
        smp._attempt(None)
        st = smp._read_state()
        ia = int(st["n_attempts"]) - 1
        check(ia, float(st["log_t"][ia]), float(st["log_h"][ia]), smp.y.cpu().numpy(), smp.Kbuf.cpu().numpy(), smp.ynew.cpu().numpy())
        if st["status"] != 0:
            break
    assert st["status"] == 1
    return int(st["n_attempts"])


def test_stage_derivatives_exact_f32_field():
    """On a field the float32 network evaluates exactly (rk45_reference.exact_f32_problem), each stage derivative of the device is
    -g^2/2 . float32(float32(A . float32(y_s)) / float32(sigma32 + 1e-7)) with y_s rebuilt from the device's own K - to within the
    rounding of that one division (u) and of sigma (powf here and on the host may differ by an ulp: 4 u) - 5 u in all.  A Dormand-Prince
    coefficient off by 1e-6 moves a stage state by 1e-6 h |K|, i.e. 1e-6 |h a A| relative: far outside 5 u on the stages where |h a A| > 0.3
    (measured: the correct library reaches 0.88 of the bound, one with DP_A[3][1] off by 1e-6 4.9)."""
    anet = rr.exact_f32_problem()
    from genpose_amd.scorenet import ScoreNetHIP
    snet = ScoreNetHIP(anet.state_dict(go.make_state_dict(0, "score")), "cuda")
    B, K, T0 = 2, 50, 1.0
    cvec, x, _, c_rows, fld, Y0 = _problem(anet, snet, "score", B, K, T0)
    fld.Y0, fld.cvec = Y0, cvec
    A = np.diag(anet.A)
    for plan in (16, 32, 64, 128, 16 | 0x100):
        worst = [0.0]

        def check(ia, t, h, y, Kd, ynew):
            for s in range(7):
                ys = y + h * (Kd[:s].T @ rr.DP_A[s, :s]) if s < 6 else ynew
                ts = t + rr.DP_C[s] * h if s < 6 else t + h
                t32 = np.float32(ts)
                sig = np.float32(np.float32(0.01) * np.power(np.float32(5000.0), t32)) + np.float32(1e-7)
                q = (np.tile(A, ys.size // 9) * ys.astype(np.float32).astype(np.float64)).astype(np.float32)
                pred = -0.5 * rr.g2(ts) * (q / sig).astype(np.float64)
                r = np.max(np.abs(Kd[s] - pred) / (5 * rr.U32 * np.abs(pred) + 1e-300))
                worst[0] = max(worst[0], r)
                assert r <= 1.0, f"plan {plan:#x} attempt {ia} stage {s}: K off by {r:.2f} x 5 u"

        n = _stage_walk(snet, fld, B, K, T0, plan, check)
        print(f"exact-field stage derivatives plan {plan:#x}: worst {worst[0]:.3f} of 5 u over {n} attempts")


def test_stage_derivatives_without_graphs():
    """One attempt at a time (no graphs): when an attempt ends, Kbuf holds its seven stage derivatives (stage 1 of the NEXT attempt
    commits y_new / K6), y its start state and ynew its end state.  Each stage derivative must be the float64 field at the stage state
    rebuilt from the device's own K - this pins the stage times, their time embedding and every tableau row."""
    anet, model, snet = _net("time")
    B, K, T0 = 2, 20, 1.0
    cvec, x, _, c_rows, fld, Y0 = _problem(anet, snet, model, B, K, T0)
    for plan in (16, 32, 64, 16 | 0x100):
        smp = _sampler(snet, model, B, K, plan, use_graph=False, poll=1)
        if smp is None:
            continue
        R = B * K
        smp.cvec.copy_(cvec)
        smp.centre.zero_()
        smp.y.copy_(torch.from_numpy(Y0.reshape(-1)).cuda())
        smp._phase(0, None, t0=T0, t_bound=rr.EPS, rtol=1e-5, atol=1e-5)
        smp._phase(1, None)
        smp._phase(2, None)
        worst = 0.0
        for i in range(200):
            smp._attempt(None)
            st = smp._read_state()
            ia = int(st["n_attempts"]) - 1
            t, h = float(st["log_t"][ia]), float(st["log_h"][ia])
            y = smp.y.cpu().numpy()
            Kd = smp.Kbuf.cpu().numpy()
            ynew = smp.ynew.cpu().numpy()
            for s in range(7):
                ys = y + h * (Kd[:s].T @ rr.DP_A[s, :s]) if s < 6 else y + h * (Kd[:6].T @ rr.DP_B)
                ts = t + rr.DP_C[s] * h if s < 6 else t + h
                if s == 6:
                    assert np.all(np.abs(ynew - ys) <= 1e-14 * (np.abs(ys) + np.abs(h) * np.abs(Kd[:6]).T @ np.abs(rr.DP_B))), (plan, i)
                    ys = ynew
                ref = fld(ts, ys.reshape(R, 9)).reshape(-1)
                bnd = fld.bound(ts, ys.reshape(R, 9)).reshape(-1)
                r = np.max(np.abs(Kd[s] - ref) / bnd)
                worst = max(worst, r)
                assert r <= 1.0, f"plan {plan:#x} attempt {ia} stage {s}: K off by {r:.2f} x its float32 bound"
            if st["status"] != 0:
                break
        print(f"stage derivatives plan {plan:#x}: worst {worst:.3f} of the bound over {int(st['n_attempts'])} attempts")
        assert st["status"] == 1


# ----------------------------------------------------------------------------- replay on network weights (chaotic solves)
WEIGHT_PLANS = (16, 32, 64, 16 | 0x100)  # 2 clouds x 10 candidates: the 128-row chain needs k >= 43, the shared plans one batch of many clouds


def _replay_weights(sd, g, case, tag):
    from genpose_amd.encoder import Pointnet2EncoderHIP
    from genpose_amd.scorenet import ScoreNetHIP
    B, K = g["pts"].shape[0], int(g["K"])
    pts = torch.from_numpy(g["pts"]).cuda()
    feat = Pointnet2EncoderHIP(sd, "cuda").forward(pts)
    snet = ScoreNetHIP(sd, "cuda")
    cvec = snet.cloud_embed(feat)
    T0 = float(g[f"{case}_T0"])
    x0 = torch.from_numpy(g[f"{case}_prior_noise"]) * go.ve_sigma(T0)  # the oracle's prior draw (genpose_oracle.pred_func), float32
    if f"{case}_init_x" in g:
        x0 = torch.from_numpy(g[f"{case}_init_x"]).unsqueeze(1).repeat(1, K, 1).reshape(B * K, -1) + x0
    Y0 = x0.double().numpy()
    fld = rr.NetField(sd, feat.cpu().numpy(), K)
    for plan in WEIGHT_PLANS:
        smp = _sampler(snet, "score", B, K, plan)
        run = rr.solve_raw(smp, cvec, torch.from_numpy(Y0).cuda(), T0, rr.EPS)[0]
        worst = rr.replay_check(fld, run, T0, rr.EPS)
        print(f"replay {tag} {case} plan {plan:#x} ({int(run['n_attempts'])} attempts): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("case", ["T1_none", "T055_none", "T015_warm"])
def test_replay_seed0_weights_g6_problems(golden, case):
    """the g6_ode.npz problems (seed-0 random weights, the logged priors, T0 = 1, 0.55 and the warm-started 0.15): every attempt, the
    late ones that test_gpu_sampler.py::test_ode_golden cannot hold to the reference's schedule included, replayed in float64"""
    _replay_weights(go.make_state_dict(0, "score"), golden("g6_ode.npz"), case, "seed-0")


def test_replay_trained_checkpoint(golden):
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trained", "ckpt_score.pth")
    sd = {k: v.float() for k, v in torch.load(path, map_location="cpu")["model_state_dict"].items()}
    _replay_weights(sd, golden("g6_ode.npz"), "T055_none", "trained")


def test_expected_skips_are_refusals():
    """every skip listed in EXPECTED_SKIPS is a refusal of the driver at that shape (and _sampler asserts nothing else is skipped)"""
    for (model, plan, B, K, groups), why in EXPECTED_SKIPS.items():
        assert _refusal(model, plan, groups, B // groups, K) == why, (model, plan, B, K, groups)


# ----------------------------------------------------------------------------- ranking on non-finite energies
def test_rank_nonfinite_energies_follow_torch_sort():
    """NaN, +-inf and +-0 energies: the ranking is torch.sort(descending=True, stable=True)'s permutation exactly (NaNs first in index
    order, then +inf, ..., -inf; -0.0 ties +0.0 in index order), and the sorted copies follow it."""
    from genpose_amd import reward
    gen = torch.Generator().manual_seed(11)
    specials = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 1.0, -1.0])
    for B, K in [(1, 1), (2, 7), (3, 50), (2, 130)]:
        pick = torch.randint(0, len(specials) + 1, (B, K, 2), generator=gen)
        energy = torch.where(pick < len(specials), specials[pick.clamp(max=len(specials) - 1)], torch.randn(B, K, 2, generator=gen))
        poses = torch.randn(B, K, 9, generator=gen, dtype=torch.float64)
        r = reward.rank_aggregate(poses.cuda(), energy.cuda(), ratio=0.6)
        order = r["order"].cpu().long()
        for c in range(2):
            ref = torch.sort(energy[:, :, c], dim=1, descending=True, stable=True)
            assert torch.equal(order[:, :, c], ref.indices), (B, K, c)
            got_e = r["sorted_energy"][:, :, c].cpu()
            assert torch.equal(torch.isnan(got_e), torch.isnan(ref.values))
            same = torch.isnan(got_e) | (got_e.view(torch.int32) == ref.values.view(torch.int32))
            assert bool(same.all())
        bi = torch.arange(B).unsqueeze(1)
        want = poses[bi, order[:, :, 0]].clone()
        want[:, :, 6:] = poses[bi, order[:, :, 1]][:, :, 6:]
        assert torch.equal(r["sorted_poses"].cpu(), want)
        assert bool(torch.isfinite(r["avg_pose"]).all())
