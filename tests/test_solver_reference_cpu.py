"""No GPU: the dtype-generic restatements of the fixed-step solvers (tests/solver_reference.py) and the conditions that the float64 gate
of tests/test_gpu_solver_f64.py places on the REFERENCE alone.

  1. The equalities.  In float64 heun_solve / dpm2m_solve / denoise / finish return what heun_reference.py / dpm2m_reference.py return,
     bit for bit; in float32 pc_solve returns what go.pc_sampler returns on the same noise, bit for bit (the operation order is kept).
     realisations(): realisation 0 is the case's x0, every other one moves EVERY element by exactly one float32 ulp, both ways occur.
  2. The conditions, on every case: the worst realisation of the fp32 restatement within SPREAD_LIMIT = 2 x the worst of the other seven
     in every output and block; E_oracle under the solver's ceiling; at most one case in four of a (solver, model, T0) group dropped.
  3. The gap.  The mutants of the sensitivity study applied to the FLOAT64 restatement: on every admitted Heun / DPM-Solver++(2M) case at
     T0 <= 0.55 the wrong corrector weight, the scaled wp and g from sigma_{N-1} exceed MARGIN x E_oracle in some output and block, and the
     two subtle ones stay under rtol = atol = 1e-3 on the weights and T0 the existing tests run (score model, seed 0).  Measured: the
     corrector weight 72x - 2 500x E_oracle at 0.06 - 0.51 of the old bound, wp 53x - 2 000x at 0.04 - 0.93.  'h_f32' (h formed from
     float32 sigmas) moves a solve by 0.01 - 0.04 of E_oracle: no accuracy gate of any margin can see it, only the equality of the
     schedule table with the float64 coefficients rounded once (asserted below on the host schedule, in the GPU file on the device's
     table).  'pc_snr' is not asserted here: PC runs from T0 = 1, where on the float64 restatement it reaches 3.8x - 4.4x E_oracle
     on the score model and 0.6x - 1.05x on the energy model (profiles/solver_f64_gate.txt); the device run of that mutant fails the GPU file."""
import numpy as np
import pytest
import torch

from oracle import genpose_oracle as go

import dpm2m_reference as dr
import f64_reference as fr
import heun_reference as hr
import solver_reference as sr

FIXED = sr.fixed_step_cases("score") + sr.SHORT_CASES + sr.fixed_step_cases("energy")
PC = list(sr.PC_CASES.values())
ids = lambda c: "-".join(str(v) for v in c)


@pytest.mark.parametrize("solver,n,grid,T0", [("heun", 6, "geometric", 0.55), ("heun", 1, "edm", 0.15), ("dpm2m", 6, "edm", 1.0), ("dpm2m", 2, "geometric", 0.55)])
def test_float64_equals_the_existing_restatements_bit_for_bit(solver, n, grid, T0):
    case = sr.Case(solver, "score", "seed0", 3, 5, T0, grid, n)
    _, centre, x0 = sr.inputs(case)
    score = sr._numpy_score(sr.network(case, torch.float64), torch.float64)
    old = hr.heun_solve if solver == "heun" else dr.dpm2m_solve
    new = sr.heun_solve if solver == "heun" else sr.dpm2m_solve
    xs_old = old(score, x0.double().numpy(), n, T0=T0, kind=grid, t32=True)
    xs_new = new(score, x0.double().numpy(), n, T0=T0, kind=grid)
    assert xs_new.dtype == np.float64 and np.array_equal(xs_new, xs_old)
    den_old, den_new = hr.denoise(score, xs_old[-1], n, t32=True), sr.denoise(score, xs_new[-1], n)
    assert np.array_equal(den_new, den_old)
    cen_r = sr.centre_rows(case).double().numpy()
    assert np.array_equal(sr.finish(xs_new[1:], cen_r), hr.finish(xs_old[1:], cen_r)) and np.array_equal(sr.finish(den_new, cen_r), hr.finish(den_old, cen_r))
    out = sr.solve(case, torch.float64)
    assert np.array_equal(out["traj"], hr.finish(xs_old[1:], cen_r)) and np.array_equal(out["pose"], hr.finish(den_old, cen_r)) and np.array_equal(out["x"], xs_old[-1])
    # and the float32 solve is a float32 solve: every state in float32, close to and different from the float64 one
    out32 = sr.solve(case, torch.float32)
    assert all(a.dtype == np.float32 for a in out32.values())
    assert not np.array_equal(out32["x"].astype(np.float64), out["x"]) and np.allclose(out32["x"], out["x"], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("model", ["score", "energy"])
def test_float32_pc_equals_the_oracles_pc_sampler_bit_for_bit(model):
    case = sr.Case("pc", model, "seed0", 3, 5, 1.0, None, 6)
    _, _, x0 = sr.inputs(case)
    z1, z2 = sr.pc_noise(case)
    cen_r = sr.centre_rows(case)
    want_xs, want_mean = go.pc_sampler(sr.network(case, torch.float32), x0, cen_r, case.n, z1, z2)
    got = sr.solve(case, torch.float32)
    assert got["xs"].dtype == np.float32 and np.array_equal(got["xs"], want_xs.numpy()) and np.array_equal(got["mean_x"], want_mean.numpy())
    ref = sr.solve(case, torch.float64)
    assert ref["xs"].dtype == np.float64 and max(max(v) for v in sr.errors(got, ref, case).values()) < 1e-3
    # two batches: each is the sampler on its own rows
    both = sr.Case("pc", model, "seed0", 4, 4, 1.0, None, 4, 11, 2)
    _, _, xb = sr.inputs(both)
    zb1, zb2 = sr.pc_noise(both)
    cb = sr.centre_rows(both)
    feat_r = sr.inputs(both)[0].repeat_interleave(both.K, 0)
    sd = fr.state_dict("seed0", model)
    half = slice(8, 16)
    fn = (lambda x, t: go.score_forward(sd, feat_r[half], x, t)) if model == "score" else (lambda x, t: go.energy_score(sd, feat_r[half], x, t)[0])
    want = go.pc_sampler(fn, xb[half], cb[half], both.n, zb1[:, half], zb2[:, half])
    got = sr.solve(both, torch.float32)
    assert np.array_equal(got["xs"][half], want[0].numpy()) and np.array_equal(got["mean_x"][half], want[1].numpy())


def test_realisations_move_every_element_by_one_ulp():
    case = FIXED[0]
    x0 = sr.inputs(case)[2]
    rs = sr.realisations(case)
    assert len(rs) == sr.R_REALISATIONS and rs[0] is x0
    ulp = (torch.nextafter(x0.abs(), torch.full_like(x0, float("inf"))) - x0.abs()).double()
    for j, x in enumerate(rs[1:], 1):
        d = x.double() - x0.double()
        assert x.dtype == torch.float32 and bool((d != 0).all()) and bool((d > 0).any()) and bool((d < 0).any())
        assert bool((d.abs() <= ulp).all()) and bool((d.abs() >= ulp / 2).all()), j  # (one ulp down from a power of two is half as far)
        assert all(not torch.equal(x, y) for y in rs[:j])


def test_block_metric_takes_the_centre_out_of_finished_translations_only():
    case = FIXED[0]
    ref = sr.reference(case)
    cen = sr.centre_rows(case).double().numpy()
    got = {k: np.array(v) for k, v in ref.items()}
    got["pose"][:, 6:9] += 1e-6
    got["x"][:, 6:9] += 1e-6
    e = sr.errors(got, ref, case)
    assert e["pose"][:2] == [0.0, 0.0] and e["x"][:2] == [0.0, 0.0] and e["traj"] == [0.0] * 3
    assert np.isclose(e["pose"][2], 1e-6 / np.abs(ref["pose"][:, 6:9] - cen).max(), rtol=1e-6)
    assert np.isclose(e["x"][2], 1e-6 / np.abs(ref["x"][:, 6:9]).max(), rtol=1e-6)
    assert np.allclose(ref["last"][:, 6:9] - cen, ref["x"][:, 6:9], rtol=0, atol=1e-15)  # (the finish adds the centre and nothing else there)


@pytest.mark.parametrize("case", FIXED + PC, ids=ids)
def test_the_reference_meets_its_own_conditions(case):
    """spread <= 2 and E_oracle under the ceiling on every admitted case; a dropped case must break the spread condition"""
    sp, E = sr.spread(case), sr.e_oracle(case)
    worst = max(max(v) for v in E.values())
    print(f"solver-oracle | {ids(case)} | spread {sp:.2f} | E_oracle max {worst:.2e} of ceiling {sr.ceiling(case):g} | "
          + " ".join(f"{n} " + "/".join(f"{e:.1e}" for e in v) for n, v in E.items()))
    if case in sr.DROPPED:
        assert sp > sr.SPREAD_LIMIT or worst >= sr.ceiling(case), "a case is dropped only where the reference breaks a condition"
        return
    assert sp <= sr.SPREAD_LIMIT
    assert all(0 < e < sr.ceiling(case) for v in E.values() for e in v)


def test_at_most_one_case_in_four_of_a_group_is_dropped():
    groups = {}
    for c in FIXED + PC:
        groups.setdefault(sr.group_of(c), []).append(c in sr.DROPPED)
    assert all(c in FIXED + PC for c in sr.DROPPED)
    for g, flags in groups.items():
        assert sum(flags) <= sr.DROP_SHARE * len(flags), (g, sum(flags), len(flags))
    assert all(c.seed == 11 or tuple(c[:8]) in sr.SEEDS for c in FIXED)


APPLIES = {"heun": ("heun_weight", "denoise_g", "h_f32"), "dpm2m": ("dpm_wp", "denoise_g")}
LOW = [c for c in sr.admitted(FIXED) if c.T0 <= 0.55]


def _mutant(case, m):
    """-> (the mutant's worst block error / E_oracle over outputs and blocks, its distance in units of the old bound)"""
    ref, E = sr.reference(case), sr.e_oracle(case)
    got = sr.solve(case, torch.float64, mutant=m)
    err = sr.errors(got, ref, case)
    return max(e / eo for n in err for e, eo in zip(err[n], E[n])), sr.old_ratio(got, ref)


@pytest.mark.parametrize("case", LOW, ids=ids)
def test_the_mutants_fall_between_the_new_gate_and_the_old_bound(case):
    for m in APPLIES[case.solver]:
        ratio, old = _mutant(case, m)
        print(f"solver-mutant | {m:11s} | {ids(case)} | {ratio:10.2f} x E_oracle | {old:.3e} of the old bound")
        if m == "h_f32":
            assert ratio < 1.0  # below the oracle's own error: the schedule equality is what sees it
            continue
        assert ratio > fr.MARGIN
        if m != "denoise_g" and case.model == "score" and case.weights == "seed0":  # the existing tests' weights
            assert old < 1.0


def _emulated(case, **kw):
    """-> (worst cell of the chained fp32 restatement over E_oracle, two realisations; its raw-state block errors on the case's own x0)"""
    ref, E, net = sr.reference(case), sr.e_oracle(case), sr.chain_network(case, **kw)
    errs = [sr.errors(sr.solve(case, torch.float32, x0, net=net), ref, case) for x0 in sr.realisations(case, 2)]
    return max(e / eo for err in errs for n in err for e, eo in zip(err[n], E[n])), errs[0]["x"]


# (case, emulation / E_oracle measured where the cases were chosen, device / E_oracle of the same case on an MI355X)
EMULATED = [
    (("heun", "score", "trained", 3, 5, 0.15, "edm"), 8.3, 7.86),
    (("dpm2m", "score", "trained", 3, 5, 0.15, "geometric"), 6.4, 7.25),
    (("heun", "score", "trained", 3, 23, 0.15, "geometric"), 3.3, 6.35),
    (("heun", "score", "trained", 3, 50, 0.15, "edm"), 6.0, 5.33),
    (("dpm2m", "score", "trained", 3, 50, 0.15, "geometric"), 4.9, 4.97),
    (("heun", "score", "seed1", 3, 50, 0.15, "edm"), 4.3, 3.58),
    (("heun", "energy", "trained", 3, 5, 0.55, "edm"), 5.7, 3.62),
    (("heun", "energy", "trained", 3, 7, 0.55, "geometric"), 4.1, 5.32),
    (("dpm2m", "energy", "trained", 3, 50, 0.55, "edm"), 3.5, 5.84),
]
DEVICE_X = (7.18e-7, 5.11e-7, 2.46e-6)  # the raw state's block errors of EMULATED[0] on an MI355X (heun_step_kernel<16>)


@pytest.mark.parametrize("key,quoted,device", EMULATED, ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_the_exceptions_cause_is_the_cloud_embeddings_chain(key, quoted, device):
    """The cause of test_gpu_solver_f64.EXCEPTIONS as a HOST EMULATION, on the shapes, models and weights the exceptions are granted
    for: the fp32 restatement with ONE thing changed - the cloud embedding (W[:, :1024] . features, which every plan consumes) summed as
    one k-ordered chain of fused multiply-adds, every per-row dot product left to the oracle's sgemm (chain_network(block=1,
    rows_block=0)).  It stays within a factor 2 of the figure quoted beside it (the band is for another host's sgemm, which moves
    E_oracle), and chaining every other dot product as well changes it by less than a third: the cloud embedding's chain is the whole
    effect, which is why tile, MFMA-chain and split-bf16 plans - and the energy model's vector-Jacobian forms - measure alike.  The
    device side of the same statement is test_gpu_solver_f64.test_the_exceptions_are_the_cloud_embeddings_chain, which gives the kernels
    an exact cloud embedding and finds every exception under 3.  Quoted 8.3x on the first case is above MARGIN_CAP: the device measures
    7.86x there, 2 % under its gate of 8, on the host that recorded it."""
    case = sr.make_case(key[0], key[1], *key[2:], 6)
    cloud, x_cloud = _emulated(case, block=1, rows_block=0)
    every, _ = _emulated(case, block=1)
    print(f"solver-emulation | {'-'.join(str(v) for v in case)} | cloud embedding chained {cloud:.2f} x E_oracle | every dot product {every:.2f} | quoted {quoted} | device {device}")
    assert quoted / 2 <= cloud <= quoted * 2
    assert abs(every / cloud - 1.0) < 1.0 / 3.0
    if key == EMULATED[0][0]:
        # the raw state, block by block, against the device's own figures; and an idealised k-block of four exact products per
        # rounding does NOT explain them (2.8x): the roundings per product are what counts
        print("solver-emulation | raw state x per block: emulated " + " / ".join(f"{e:.2e}" for e in x_cloud) + " | device " + " / ".join(f"{e:.2e}" for e in DEVICE_X))
        assert all(d / 2 <= e <= d * 2 for e, d in zip(x_cloud, DEVICE_X))
        assert _emulated(case, block=4)[0] < cloud / 2


def test_on_seeded_weights_the_chain_sits_at_the_edge_of_the_margin():
    """Seed 0, 15 rows, T0 = 0.15: the same emulation is 2.7x - 3.3x E_oracle (device: 1.77 and 3.09 on the two grids), where the trained
    checkpoint is 8x: the seeded-weight exceptions (3.09 - 4.005 on the device) are this edge, not another cause."""
    trained = _emulated(sr.make_case("heun", "score", "trained", 3, 5, 0.15, "edm", 6), block=1, rows_block=0)[0]
    for grid in sr.GRIDS:
        r = _emulated(sr.make_case("heun", "score", "seed0", 3, 5, 0.15, grid, 6), block=1, rows_block=0)[0]
        print(f"solver-emulation | seed0 heun 3x5 T0=0.15 {grid}: cloud embedding chained {r:.2f} x E_oracle (trained: {trained:.2f})")
        assert 1.3 <= r <= 6.6 and r < trained


@pytest.mark.parametrize("grid", sr.GRIDS)
@pytest.mark.parametrize("T0", sr.T0S)
def test_the_host_schedules_are_the_restatements_coefficients_rounded_once(T0, grid):
    """What solver_reference assumes of samplers.heun_schedule / dpm2m_schedule, which its grid never comes from: h_i, sigma_i and the
    DPM-Solver++(2M) weights are the float64 values of the reference modules, rounded once ('h_f32' and 'dpm_wp' change a word here)."""
    from genpose_amd.samplers import dpm2m_schedule, heun_schedule
    N, f = sr.N_STEPS, np.float32
    t, sig, h = hr.grid(N, T0, kind=grid)
    th, sh = heun_schedule(N, T0, grid=grid)
    assert np.array_equal(th, t) and np.array_equal(sh[1:2 * N + 1:2, 2], h.astype(f)) and np.array_equal(sh[2:2 * N + 1:2, 2], h.astype(f))
    assert np.array_equal(sh[1:2 * N + 1:2, 1], (-sig[:-1]).astype(f)) and np.array_equal(sh[2:2 * N + 1:2, 1], (-sig[1:]).astype(f))
    s2, ratio, wc, wp = dr.coefficients(sig)
    td, sd = dpm2m_schedule(N, T0, grid=grid)
    assert np.array_equal(td, t)
    for col, want in ((1, s2), (2, ratio), (4, wc), (5, wp)):
        assert np.array_equal(sd[1:N + 1, col], want.astype(f)), col
    # the restatement's own coefficients are those: wc = -expm1(-h) (1 + 1/(2r)), wp = expm1(-h) / (2r), to float64 rounding
    lam = -np.log(sig)
    hh = lam[1:] - lam[:-1]
    r = (lam[1:-1] - lam[:-2]) / hh[1:]
    assert np.allclose(wc[1:], -np.expm1(-hh[1:]) * (1.0 + 1.0 / (2.0 * r)), rtol=1e-15, atol=0) and np.allclose(wp[1:], np.expm1(-hh[1:]) / (2.0 * r), rtol=1e-15, atol=0)
    assert sh[2 * N + 1, 1] == sd[N + 1, 1] and abs(float(sh[2 * N + 1, 1]) / (hr.sigma(hr.EPS) * hr.G_FACTOR) - 1) < 2e-7  # g(eps), formed in float32
