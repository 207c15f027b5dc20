"""The fixed-step solvers restated with the working dtype as a parameter, and the float64 gate built on them (helper of
test_solver_reference_cpu.py and test_gpu_solver_f64.py; CPU only, nothing here touches a device or imports genpose_amd).

    heun_solve / dpm2m_solve / denoise / finish
                    heun_reference.py's and dpm2m_reference.py's loops in their operation order, every operation in `dtype`.  The grid is
                    heun_reference.grid's; the grid and every coefficient are computed in float64 and rounded ONCE to `dtype` (what
                    samplers.heun_schedule / dpm2m_schedule promise); the network sees the float32 time (t32=True).  In float64 they return
                    what the existing restatements return, bit for bit (np.array_equal, test_solver_reference_cpu.py): the expressions are
                    the same ones, a coefficient rounded "to float64" is itself.
    pc_solve        go.pc_sampler with the dtype as a parameter, the operation order kept: in float32 it equals go.pc_sampler bit for bit.
                    The times are the float32 linspace the device is given, in either precision.  groups > 1: every batch on its own
                    (the batch mean of the gradient norm stays per batch).
    Case            one solve: solver, model, weights, shape, T0, grid, N, input seed (and the batches of a PC run)
    solve(case, dtype, x0=None, mutant=None)
                    {output: array} of a case in `dtype` - 'traj' (x_1 .. x_N finished), 'last' (x_N finished), 'pose' (the denoised x_N
                    finished), 'x' (x_N raw) for Heun / DPM-Solver++(2M); 'xs', 'mean_x' for PC
    realisations(case, r)
                    r float32 starting states: 0 is the case's own, j > 0 moves every element of x0 by one float32 ulp up or down by a
                    seeded coin; nothing else changes.  Every realisation is compared with the float64 solve of the UNPERTURBED inputs.
    errors(got, ref, case)
                    f64_reference.block_error per block (0:3, 3:6, 6:9) and output.  On finished outputs the cloud-centre rows are first
                    subtracted from the translation block of both sides (a centre of 0.3 would otherwise set the scale at T0 = 0.15); the
                    raw state 'x' is compared as it is.
    e_oracle(case)  THE YARDSTICK: per output and block the maximum over R = 8 realisations of the fp32 restatement's error.  It never
                    sees the code under test.

THE RULE (tests/test_gpu_solver_f64.py).  A device result passes at block_error <= MARGIN x E_oracle with f64_reference.MARGIN = 3, named
exceptions by that module's rule (one demonstrated cause, the next power of two, never above MARGIN_CAP = 8).  3 carries over from the
single evaluations because the solves are recursions of those evaluations; on the admitted cases one realisation exceeds the maximum of the
others by 1.0x to 1.6x under one sgemm blocking and thread count and by at most 1.9x under another.  That spread is a property of the
CPU's fp32 arithmetic: about one case in thirty crosses a condition on one CPU and not on another, which is why the draws of SEEDS and
PC_CASES were checked on two.

CONDITIONS ON THE REFERENCE ALONE, asserted in test_solver_reference_cpu.py:
  - a case is admitted only if every realisation is at most SPREAD_LIMIT = 2 x the maximum of the other seven, in every output and block
    (spread()); a case that breaks this is DROPPED by name with its figure, at most one case in four of a (solver, model, T0) group;
  - E_oracle stays under ceiling(case) in every admitted cell (chosen under SEED_HEADROOM x that on the host that chose the cases).

MUTANTS (solve(..., mutant=)): the five subtle errors of the sensitivity study, applied to the float64 restatement on the host -
'heun_weight' (the corrector's 0.5 d' -> 0.50005 d'), 'dpm_wp' (the weight of D_{i-1} times 1 + 1e-4), 'pc_snr' (0.48 -> 0.48005),
'denoise_g' (g from sigma_{N-1}), 'h_f32' (Heun's h from float32 sigmas)."""
import collections
import functools

import numpy as np
import torch

from oracle import genpose_oracle as go

import f64_reference as fr
import heun_reference as hr
from test_gpu_heun import _inputs as _heun_inputs

EPS = hr.EPS
R_REALISATIONS = 8
SPREAD_LIMIT = 2.0       # a realisation against the maximum of the other seven
DROP_SHARE = 0.25        # of a (solver, model, T0) group
SEED_HEADROOM = fr.SEED_HEADROOM
# E_oracle's ceiling per solver, a condition on the reference alone: every admitted cell stays under SEED_HEADROOM x this on the host
# that chose the cases (the headroom is for another host's fp32 rounding).  Measured worst admitted cell beside each.  The fixed-step
# solvers have two: up to T0 = 0.55, the regime the accuracy claim is about, and T0 = 1, where the flow of the trained score network
# amplifies fp32 rounding of the score a thousandfold (the fp32 restatement itself is then 1e-3 from float64 on finished rotations, at
# the old bound: the gate is no tighter there than the oracle is, and says so in its table).
CEILING = {("heun", "low"): 2e-4,    # measured 7.1e-5 (trained score weights, 3 x 50, T0 = 0.55, edm: a finished rotation block; raw state 2.6e-5)
           ("heun", "high"): 2e-2,   # measured 6.4e-3 (trained score weights, 3 x 50, T0 = 1, edm)
           ("dpm2m", "low"): 2e-4,   # measured 5.9e-5 (trained energy weights, 3 x 50, T0 = 0.55, edm)
           ("dpm2m", "high"): 2e-2,  # measured 1.3e-3 (trained score weights, 3 x 50, T0 = 1, edm)
           ("pc", "high"): 4e-4}     # measured 1.24e-4 (score model, 3 x 23: a rotation block after Gram-Schmidt; translation 1.7e-6)


def ceiling(case):
    return CEILING[case.solver, "low" if case.T0 <= 0.55 else "high"]


MUTANTS = ("heun_weight", "dpm_wp", "pc_snr", "denoise_g", "h_f32")
OLD_BOUND = 1e-3         # rtol = atol of the existing solver tests

Case = collections.namedtuple("Case", "solver model weights B K T0 grid n seed groups", defaults=(11, 1))


# ----------------------------------------------------------------------------- inputs and networks
@functools.lru_cache(maxsize=None)
def inputs(case):
    """features [B,1024], centres [B,3], x0 [B K,9] = N(0, sigma(T0)^2): test_gpu_heun._inputs' draw (float32, read-only)"""
    return _heun_inputs(case.B, case.K, case.T0, case.seed)


@functools.lru_cache(maxsize=None)
def pc_noise(case):
    """the two injected draws of every PC step, [n, R, 9] float32 each"""
    g = torch.Generator().manual_seed(7000 + 100 * case.seed + case.B * case.K + case.n)
    R = case.B * case.K
    return torch.randn(case.n, R, 9, generator=g), torch.randn(case.n, R, 9, generator=g)


def network(case, dtype, rows=slice(None)):
    """score(x [R,9] tensor, t [R,1] tensor) -> [R,9] in `dtype`: go.score_forward, or the gradient of the inner-product energy"""
    sd = (fr.state_dict64 if dtype == torch.float64 else fr.state_dict)(case.weights, case.model)
    feat_r = inputs(case)[0].repeat_interleave(case.K, 0)[rows].to(dtype)
    if case.model == "score":
        return lambda x, t: go.score_forward(sd, feat_r, x, t)
    return lambda x, t: go.energy_score(sd, feat_r, x, t)[0]


def _linear_chain(x, W, b, block=1):
    """x [R,K] . W [O,K]^T + b in float32 the way a matrix-pipe kernel sums it: ONE accumulator per output, k in order, one rounding per
    `block` products (1: a chain of fused multiply-adds; 4: an idealised MFMA k-block whose four products are summed exactly) - where the
    oracle's sgemm spreads the sum over vector lanes and k-blocks.  block = 0: the oracle's own F.linear (a part left unchained)."""
    if block == 0:
        return torch.nn.functional.linear(x, W) + b
    x, W = x.numpy().astype(np.float64), W.numpy().astype(np.float64)
    acc = np.zeros((x.shape[0], W.shape[0]), dtype=np.float32)
    for k in range(0, x.shape[1], block):
        acc = (acc + x[:, k:k + block] @ W[:, k:k + block].T).astype(np.float32)  # (products of float32 are exact in float64)
    return torch.from_numpy(acc) + b


def chain_network(case, block=1, rows_block=None):
    """HOST EMULATION OF THE DEVICE'S ACCUMULATION ORDER (float32, either model): the oracle's network with every dot product summed by
    _linear_chain, the heads' first layer split the way the kernels split it (cloud part once per cloud, time part once per time, pose
    part per row).  Everything else - the operations, their order, sin / cos, the divisions by sigma - is the oracle's.  Score model:
    go.score_forward.  Energy model: go.energy_score's gradient f / sigma + J_f^T (x / sigma), the vector-Jacobian product written out
    layer by layer (the ReLU masks of the chained forward pass, every product v . W a chain over the layer's outputs).
    block: products per rounding of the cloud embedding's chain; rows_block: of every per-row and per-time dot product (default: block;
    0 leaves those to the oracle's sgemm, so that the cloud embedding ALONE is chained)."""
    rb = block if rows_block is None else rows_block
    sd = fr.state_dict(case.weights, case.model)
    w = lambda k: sd[fr.P + k]
    Wa = torch.cat([w(f"fusion_tail_{h}.0.weight") for h in fr.HEADS], 0)
    ba = torch.cat([w(f"fusion_tail_{h}.0.bias") for h in fr.HEADS], 0)
    W2 = [w(f"fusion_tail_{h}.2.weight") for h in fr.HEADS]
    lin = lambda x, W, b: _linear_chain(x, W, b, rb)
    cvec = _linear_chain(inputs(case)[0], Wa[:, :1024], torch.zeros(768), block).repeat_interleave(case.K, 0)
    tvec = {}

    def score(x, t):
        key = float(t[0, 0])
        if key not in tvec:
            xp = t[:1, 0][:, None] * w("t_encoder.0.W")[None, :] * 2 * np.pi
            tf = torch.relu(lin(torch.cat([torch.sin(xp), torch.cos(xp)], dim=-1), w("t_encoder.1.weight"), w("t_encoder.1.bias")))
            tvec[key] = lin(tf, Wa[:, 1024:1152], torch.zeros(768))
        z0 = lin(x, w("pose_encoder.0.weight"), w("pose_encoder.0.bias"))
        z1 = lin(torch.relu(z0), w("pose_encoder.2.weight"), w("pose_encoder.2.bias"))
        za = (cvec + tvec[key]) + lin(torch.relu(z1), Wa[:, 1152:], ba)
        a = torch.relu(za)
        f = torch.cat([lin(a[:, 256 * i:256 * (i + 1)], W2[i], w(f"fusion_tail_{h}.2.bias")) for i, h in enumerate(fr.HEADS)], dim=-1)
        if case.model == "score":
            return f / (go.ve_sigma(t) + 1e-7)
        sigma = go.ve_sigma(t)
        v = x / sigma
        none = torch.zeros(1)
        ga = torch.cat([lin(v[:, 3 * i:3 * i + 3], W2[i].T.contiguous(), none) for i in range(3)], dim=-1) * (za > 0)
        g1 = lin(ga, Wa[:, 1152:].T.contiguous(), none) * (z1 > 0)
        g0 = lin(g1, w("pose_encoder.2.weight").T.contiguous(), none) * (z0 > 0)
        return f / sigma + lin(g0, w("pose_encoder.0.weight").T.contiguous(), none)
    return score


def _numpy_score(net, dtype):
    """score(x array, t float) -> array of x's dtype, for the numpy loops below"""
    def score(x, t):
        xt = torch.from_numpy(np.ascontiguousarray(x))
        return net(xt, torch.full((xt.shape[0], 1), t, dtype=dtype)).numpy()
    return score


def _t32(v):
    return float(np.float32(v))


# ----------------------------------------------------------------------------- Heun / DPM-Solver++(2M), dtype as a parameter
def heun_solve(score, x0, nsteps, T0=1.0, eps=EPS, kind="geometric", rho=7.0, dtype=np.float64, mutant=None):
    """heun_reference.heun_solve(t32=True) with every operation in `dtype`: all states [N+1, ...]"""
    t, sig, h = hr.grid(nsteps, T0, eps, kind, rho)
    if mutant == "h_f32":
        s32 = sig.astype(np.float32)
        h = (s32[1:] - s32[:-1]).astype(np.float64)
    sig, h = sig.astype(dtype), h.astype(dtype)
    half, wp = dtype(0.5), dtype(0.50005 if mutant == "heun_weight" else 0.5)
    x = np.asarray(x0, dtype=dtype)
    xs = [x]
    for i in range(int(nsteps)):
        d = -sig[i] * score(x, _t32(t[i]))
        xe = x + h[i] * d
        dp = -sig[i + 1] * score(xe, _t32(t[i + 1]))
        x = x + h[i] * (half * d + wp * dp)
        assert x.dtype == dtype
        xs.append(x)
    return np.stack(xs)


def dpm2m_solve(score, x0, nsteps, T0=1.0, eps=EPS, kind="geometric", rho=7.0, dtype=np.float64, mutant=None):
    """dpm2m_reference.dpm2m_solve(t32=True) with every operation in `dtype`; the per-step coefficients (sigma_i^2, the weights of D_i and
    D_{i-1}, sigma_{i+1} / sigma_i, expm1(-h_i)) in float64 by that function's expressions, rounded once"""
    t, sig, _ = hr.grid(nsteps, T0, eps, kind, rho)
    lam = -np.log(sig)
    x = np.asarray(x0, dtype=dtype)
    xs, D_prev = [x], None
    for i in range(int(nsteps)):
        h = lam[i + 1] - lam[i]
        D = x + dtype(sig[i] ** 2) * score(x, _t32(t[i]))
        if i == 0:
            Dt = D
        else:
            r = (lam[i] - lam[i - 1]) / h
            b = (1.0 / (2.0 * r)) * ((1.0 + 1e-4) if mutant == "dpm_wp" else 1.0)
            Dt = dtype(1.0 + 1.0 / (2.0 * r)) * D - dtype(b) * D_prev
        x = dtype(sig[i + 1] / sig[i]) * x - dtype(np.expm1(-h)) * Dt
        assert x.dtype == dtype
        D_prev = D
        xs.append(x)
    return np.stack(xs)


def denoise(score, x, nsteps, eps=EPS, dtype=np.float64, g_sigma=None):
    """heun_reference.denoise(t32=True) in `dtype`; g_sigma: the sigma that g is formed from (the 'denoise_g' mutant's sigma_{N-1})"""
    g = dtype((hr.sigma(float(eps)) if g_sigma is None else g_sigma) * hr.G_FACTOR)
    return x + (dtype(0.0) - g * g * score(x, _t32(eps))) * dtype((1.0 - float(eps)) / int(nsteps))


def normalize_rot6(x, dtype=np.float64):
    """heun_reference.normalize_rot6 in `dtype`"""
    x = np.array(x, dtype=dtype)
    a1, a2 = x[..., 0:3], x[..., 3:6]
    b1 = a1 / np.maximum(np.linalg.norm(a1, axis=-1, keepdims=True), dtype(1e-12))
    b2 = a2 - np.sum(b1 * a2, axis=-1, keepdims=True) * b1
    b2 = b2 / np.maximum(np.linalg.norm(b2, axis=-1, keepdims=True), dtype(1e-12))
    x[..., 0:3], x[..., 3:6] = b1, b2
    assert x.dtype == dtype
    return x


def finish(x, centre_rows, dtype=np.float64):
    """heun_reference.finish in `dtype`"""
    y = normalize_rot6(x, dtype)
    y[..., 6:9] += np.asarray(centre_rows, dtype=dtype)
    return y


# ----------------------------------------------------------------------------- PC, dtype as a parameter
def pc_solve(score_fn, init_x, pts_center, num_steps, z_langevin, z_predictor, dtype=torch.float32, snr=0.16, eps=EPS, noise_norm=None):
    """go.pc_sampler line for line, `dtype` where it says float32.  The time steps are the float32 linspace in either precision (the
    values the device's time embedding and schedule are given); step_size = t_0 - t_1 is exact in float32 for num_steps >= 3.
    noise_norm: sqrt(9) unless a mutant replaces it.  -> (xs [R,num_steps,9], mean_x [R,9]) in `dtype`"""
    x = init_x.clone().to(dtype)
    z_langevin, z_predictor, pts_center = z_langevin.to(dtype), z_predictor.to(dtype), pts_center.to(dtype)
    R = x.shape[0]
    time_steps = torch.linspace(1.0, eps, num_steps).to(dtype)
    step_size = time_steps[0] - time_steps[1]
    noise_norm = np.sqrt(9) if noise_norm is None else noise_norm
    xs = []
    mean_x = None
    for i, ts in enumerate(time_steps):
        bt = torch.ones(R, dtype=dtype).unsqueeze(-1) * ts
        grad = score_fn(x, bt)
        grad_norm = torch.norm(grad.reshape(R, -1), dim=-1).mean()
        lstep = 2 * (snr * noise_norm / grad_norm) ** 2
        x = x + lstep * grad + torch.sqrt(2 * lstep) * z_langevin[i]
        x[:, :3] /= torch.norm(x[:, :3], dim=-1, keepdim=True)
        x[:, 3:6] /= torch.norm(x[:, 3:6], dim=-1, keepdim=True)
        g = go.ve_diffusion(bt)
        drift = 0 - g ** 2 * grad
        mean_x = x + drift * step_size
        x = mean_x + g * torch.sqrt(step_size) * z_predictor[i]
        x[:, :-3] = go.normalize_rotation(x[:, :-3])
        assert x.dtype == dtype
        xs.append(x.unsqueeze(0).clone())
    xs = torch.cat(xs, dim=0)
    xs[:, :, -3:] += pts_center.unsqueeze(0)
    mean_x = mean_x.clone()
    mean_x[:, -3:] += pts_center
    mean_x[:, :-3] = go.normalize_rotation(mean_x[:, :-3])
    return xs.permute(1, 0, 2), mean_x


# ----------------------------------------------------------------------------- one case
def centre_rows(case):
    return inputs(case)[1].repeat_interleave(case.K, 0)


def solve(case, dtype, x0=None, mutant=None, net=None):
    """{output: array} of the case in `dtype` (torch.float32 / torch.float64) from x0 (default: the case's own); net: another network
    than network(case, dtype) (chain_network's emulation; fixed-step solvers only)"""
    _, centre, x_case = inputs(case)
    x0 = x_case if x0 is None else x0
    if case.solver == "pc":
        z1, z2 = pc_noise(case)
        cen_r = centre_rows(case)
        Rg = case.B * case.K // case.groups
        nn = 0.48005 / 0.16 if mutant == "pc_snr" else None
        parts = []
        for g in range(case.groups):
            rows = slice(g * Rg, (g + 1) * Rg)
            parts.append(pc_solve(network(case, dtype, rows), x0[rows], cen_r[rows], case.n, z1[:, rows], z2[:, rows], dtype, noise_norm=nn))
        return {"xs": torch.cat([p[0] for p in parts]).numpy(), "mean_x": torch.cat([p[1] for p in parts]).numpy()}
    nd = np.float64 if dtype == torch.float64 else np.float32
    score = _numpy_score(net or network(case, dtype), dtype)
    fn = heun_solve if case.solver == "heun" else dpm2m_solve
    kw = dict(mutant=mutant) if mutant in ("heun_weight", "h_f32", "dpm_wp") else {}
    xs = fn(score, x0.to(dtype).numpy(), case.n, T0=case.T0, kind=case.grid, dtype=nd, **kw)
    g_sigma = hr.grid(case.n, case.T0, EPS, case.grid)[1][-2] if mutant == "denoise_g" else None
    den = denoise(score, xs[-1], case.n, dtype=nd, g_sigma=g_sigma)
    cen_r = centre_rows(case).to(dtype).numpy()
    return {"traj": finish(xs[1:], cen_r, nd), "last": finish(xs[-1], cen_r, nd), "pose": finish(den, cen_r, nd), "x": xs[-1]}


@functools.lru_cache(maxsize=None)
def reference(case):
    """the float64 solve of the case's unperturbed inputs (cached: do not write)"""
    out = solve(case, torch.float64)
    for a in out.values():
        a.setflags(write=False)
    return out


def realisations(case, r=R_REALISATIONS):
    """r starting states [R,9] float32: the case's own, then r - 1 copies with every element one float32 ulp up or down by a seeded coin"""
    x0 = inputs(case)[2]
    out = [x0]
    for j in range(1, r):
        up = torch.rand(x0.shape, generator=torch.Generator().manual_seed(9000 + j)) < 0.5
        inf = torch.full_like(x0, float("inf"))
        out.append(torch.where(up, torch.nextafter(x0, inf), torch.nextafter(x0, -inf)))
    return out


RAW = ("x",)  # outputs compared as they are; every other output is finished (centre added) and is compared with the centre taken out


def errors(got, ref, case):
    """{output: [three block errors]} of `got` ({output: array}, any subset of the reference's outputs) against `ref`"""
    cen = centre_rows(case).double().numpy()
    out = {}
    for name, g in got.items():
        g, r = np.array(g, dtype=np.float64), np.array(ref[name], dtype=np.float64)
        if name not in RAW:
            c = cen[:, None, :] if (name == "xs") else cen
            g[..., 6:9] -= c
            r[..., 6:9] -= c
        out[name] = fr.block_error(g, r, fr.BLOCKS9)
    return out


def old_ratio(got, ref):
    """max |got - ref| / (atol + rtol |ref|) at the existing tests' rtol = atol = 1e-3 over every output: 1 is that bound"""
    return max(float((np.abs(np.asarray(g, dtype=np.float64) - ref[n]) / (OLD_BOUND + OLD_BOUND * np.abs(ref[n]))).max()) for n, g in got.items())


@functools.lru_cache(maxsize=None)
def realisation_errors(case):
    """[realisation][output][block]: the fp32 restatement's error on each of the R realisations"""
    ref = reference(case)
    return [errors(solve(case, torch.float32, x0), ref, case) for x0 in realisations(case)]


@functools.lru_cache(maxsize=None)
def e_oracle(case):
    """{output: [per block: max over the realisations]}"""
    per = realisation_errors(case)
    return {n: [max(p[n][j] for p in per) for j in range(3)] for n in per[0]}


@functools.lru_cache(maxsize=None)
def spread(case):
    """the worst, over outputs and blocks, of the largest realisation over the largest of the OTHER seven: the admission figure"""
    per = realisation_errors(case)
    worst = 0.0
    for n in per[0]:
        for j in range(3):
            e = sorted(p[n][j] for p in per)
            worst = max(worst, e[-1] / e[-2])
    return worst


# ----------------------------------------------------------------------------- the cases
N_STEPS = 6
T0S = (0.15, 0.55, 1.0)
GRIDS = ("geometric", "edm")
SCORE_SHAPES = ((3, 5), (3, 23), (3, 50))      # test_gpu_heun.PLANS: tile16 | tile32, tile64 | chain_f32, chain_bf16x9
SCORE_WEIGHTS = ("seed0", "seed1", "trained")
ENERGY_SHAPES = ((3, 5), (3, 7), (3, 50))      # fixed_step_energy_cases.SHAPES: tile16, tile16x2, chain
ENERGY_CASES = (("seed0", 0.15), ("seed0", 0.55), ("trained", 0.55))  # fixed_step_energy_cases.CASES ('random' is seed 0)
PC_STEPS = 20


# The input seed of a case is test_gpu_heun._inputs' 11 unless the REFERENCE broke a condition on that draw; then it is the first of 12,
# 13, ... on which the fp32 restatement's realisations stay within 1.6x (SEED_HEADROOM x SPREAD_LIMIT) of each other and under SEED_HEADROOM x the ceiling.  The
# figure beside each is what seed 11 gave (spread = the worst realisation over the worst of the other seven; E = the largest cell of
# E_oracle).  No kernel entered this choice.  The energy-model case with E = 8.1e-2 is one of fixed_step_energy_cases.DROPPED's three (the
# other two are DROPPED below).
SEEDS = {
    ("heun", "score", "seed0", 3, 5, 0.15, "geometric", 6): 12,    # spread 2.27 under another sgemm blocking and thread count (1.31 where the draws were first chosen)
    ("heun", "score", "seed1", 3, 23, 0.15, "geometric", 6): 12,   # spread 2.68 under the other blocking (1.40)
    ("heun", "score", "seed1", 3, 23, 0.15, "edm", 6): 12,         # spread 2.00
    ("heun", "score", "seed0", 3, 50, 1.0, "geometric", 6): 12,    # spread 2.77
    ("heun", "score", "seed0", 3, 50, 1.0, "edm", 6): 13,          # spread 1.93
    ("dpm2m", "score", "seed1", 3, 5, 1.0, "geometric", 6): 13,    # spread 1.91
    ("dpm2m", "score", "seed0", 3, 23, 0.15, "geometric", 6): 12,  # spread 2.30
    ("dpm2m", "score", "seed0", 3, 50, 1.0, "edm", 6): 13,         # spread 1.62
    ("dpm2m", "score", "trained", 3, 50, 0.55, "geometric", 6): 12,  # E 8.3e-4 (one trajectory state's Gram-Schmidt; spread 1.19)
    ("heun", "energy", "trained", 3, 5, 0.55, "edm", 6): 12,       # spread 1.65
    ("heun", "energy", "seed0", 3, 7, 0.55, "edm", 6): 12,         # spread 57.4
    ("heun", "energy", "trained", 3, 50, 0.55, "geometric", 6): 12,  # E 8.1e-2, spread 1.00
    ("dpm2m", "energy", "seed0", 3, 50, 0.15, "geometric", 6): 13,  # spread 1.71
}


def make_case(solver, model, weights, B, K, T0, grid, n, groups=1):
    return Case(solver, model, weights, B, K, T0, grid, n, SEEDS.get((solver, model, weights, B, K, T0, grid, n), 11), groups)


def fixed_step_cases(model):
    out = []
    for solver in ("heun", "dpm2m"):
        if model == "score":
            out += [make_case(solver, "score", w, B, K, T0, grid, N_STEPS) for B, K in SCORE_SHAPES for w in SCORE_WEIGHTS for T0 in T0S for grid in GRIDS]
        else:
            out += [make_case(solver, "energy", w, B, K, T0, grid, N_STEPS) for B, K in ENERGY_SHAPES for w, T0 in ENERGY_CASES for grid in GRIDS]
    return out


# N = 1 (Heun) and N = 2 (DPM-Solver++(2M): the first step that uses wp and the carried denoiser) on the 16-row tile at T0 = 0.55
SHORT_CASES = [Case("heun", "score", "seed0", 3, 5, 0.55, "geometric", 1), Case("dpm2m", "score", "seed0", 3, 5, 0.55, "geometric", 2)]
PC_CASES = {
    "score 3x5": Case("pc", "score", "seed0", 3, 5, 1.0, None, PC_STEPS),
    "score 3x23": Case("pc", "score", "seed0", 3, 23, 1.0, None, PC_STEPS, 16),    # seed 11: spread 2.17 under another sgemm blocking (1.47 where first chosen)
    "score 3x50": Case("pc", "score", "seed0", 3, 50, 1.0, None, PC_STEPS),
    "score 2x(2x8)": Case("pc", "score", "seed0", 4, 8, 1.0, None, PC_STEPS, 11, 2),
    "energy 3x5": Case("pc", "energy", "seed0", 3, 5, 1.0, None, PC_STEPS, 12),    # seed 11: spread 2.03 under another sgemm blocking (1.29 where first chosen)
    "energy 3x50": Case("pc", "energy", "seed0", 3, 50, 1.0, None, PC_STEPS, 12),  # seed 11: E 1.7e-2 under another sgemm blocking (a ReLU kink of the gradient; 2.2e-5 where first chosen)
    "score 3x50 N=100": Case("pc", "score", "seed0", 3, 50, 1.0, None, 100),
}
# Cases left out because the REFERENCE breaks a condition on them - case -> the figure.  No kernel enters this list.  Both are
# fixed_step_energy_cases.DROPPED's seed-0 energy model on 150 rows from T0 = 0.55 on the geometric grid: the energy model's score is a
# gradient and jumps at a ReLU kink, and on one row of 150 the fp32 network takes the other side of one in EVERY realisation (spread
# 1.00, so only the ceiling sees it).  Another draw does not cure it: seed 12 stays under the ceiling under one sgemm blocking (E 1.1e-4) and is
# 3.0e-3 / 3.9e-4 under another.  One case of twelve in each (solver, energy, 0.55) group.
DROPPED = {
    Case("heun", "energy", "seed0", 3, 50, 0.55, "geometric", 6): "E 1.2e-3 of a ceiling of 2e-4, spread 1.00",
    Case("dpm2m", "energy", "seed0", 3, 50, 0.55, "geometric", 6): "E 1.4e-3 of a ceiling of 2e-4, spread 1.00",
}


def admitted(cases):
    return [c for c in cases if c not in DROPPED]


def group_of(case):
    return (case.solver, case.model, case.T0)
