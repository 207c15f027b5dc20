"""cond_ode_likelihood (networks/gf_algorithms/samplers.py:22-99) - SURVEY §8f row 3.

The instantaneous change-of-variables ODE  d[x, logp]/dt = [-g(t)^2/2 * score(x, t), -g(t)^2/2 * div_x score(x, t)]  integrated from
eps to 1 with Dormand-Prince 5(4) under scipy's step controller (`integrate.solve_ivp(method='RK45')`, rtol = atol = 1e-5, one error
norm over the whole [x; logp] vector), the divergence by the Skilling-Hutchinson estimator with ONE fixed probe eps ~ prior.  The
reference runs the solver on the host: two network evaluations (one of them under autograd) and four PCIe crossings per function
call.  Here the whole solve is resident on the device - the RK45 driver of the samplers (csrc/rk45.hip, model 2) with a ten-component
state per row, score and divergence from one fused forward + vector-Jacobian pass per stage (csrc/score_bwd.h) - and the host reads
one status word per replayed chunk of attempts.

divergence='exact' (ours; not in the reference): the same ODE with the exact trace tr(d score / d x) = sum_i (e_i^T J)_i in place of the
one-probe estimate - nine unit seeds per row behind one forward pass (csrc/score_bwd.h: score_div_exact_tile; RK45 model
'likelihood_exact').  The likelihood is then a deterministic function of (cloud, pose): no probe, no draw.

solver='heun' (ours): the same exact-divergence ODE by Heun's method on a fixed sigma grid instead of the adaptive driver
(samplers.HeunLikelihood, csrc/heun_likelihood.hip): 2 N evaluations in one captured launch chain, nothing read back, row-local.
"""
import math

import torch

from .samplers import HeunLikelihood, ODESampler
from .sde import SIGMA_MAX


def global_prior_likelihood(z, sigma_max):
    """log N(z; 0, sigma_max^2 I) per row (samplers.py:13-19)."""
    n = z.shape[1]
    return -n / 2.0 * math.log(2 * math.pi * sigma_max ** 2) - torch.sum(z ** 2, dim=-1) / (2 * sigma_max ** 2)


DIVERGENCES = {"hutchinson": "likelihood", "exact": "likelihood_exact"}  # divergence= -> the ODESampler model that integrates it


def solver_model(divergence):
    """The ODESampler model behind a `divergence` value; an unknown value is refused by name."""
    if divergence not in DIVERGENCES:
        raise NotImplementedError(f"divergence {divergence!r}: 'hutchinson' (the reference's one-probe estimate) or 'exact' (the trace itself)")
    return DIVERGENCES[divergence]


SOLVERS = ("rk45", "heun")


def cond_ode_likelihood(net, cvec, k, x, epsilon=None, eps=1e-5, rtol=1e-5, atol=1e-5, stats=None, solver=None, divergence="hutchinson", steps=None,
                        grid="geometric"):
    """net: ScoreNetHIP; cvec [B,768] (gp_cloud_embed); x [B*k,9] poses whose likelihood is wanted; epsilon [B*k,9] the fixed
    Hutchinson probe (the reference draws it from the prior, samplers.py:39).  Returns (z [R,9], log-likelihood in bits [R] f64)
    on the device (z: f64 under 'rk45', the solver's f32 state under 'heun').
    divergence: 'hutchinson' (default: the reference's estimator, needs epsilon) or 'exact' (the trace itself; epsilon must be None).
    solver: 'rk45' (default, also None: the adaptive Dormand-Prince driver at rtol / atol), 'heun' (ours: the fixed-step Heun solve in
    sigma, samplers.HeunLikelihood - `steps` = its N, `grid` its sigma grid; needs divergence='exact'; rtol / atol are not used; row-local:
    a row's value does not depend on the other rows of the call), or a solver OBJECT of the right shape to reuse (buffers, captured
    launches): an ODESampler of the right model, or a HeunLikelihood (its own steps and grid hold).
    stats: 'nfev' (heun: 2 N) and 'attempts' (heun: N, the steps)."""
    model = solver_model(divergence)
    if solver is None or isinstance(solver, str):
        method, solver = ("rk45" if solver is None else solver), None
        if method not in SOLVERS:
            raise NotImplementedError(f"likelihood solver {method!r}: one of {SOLVERS}")
    else:
        method = "heun" if isinstance(solver, HeunLikelihood) else "rk45"
    if method == "heun" and divergence != "exact":
        raise NotImplementedError(f"solver='heun' with divergence={divergence!r}: the fixed-step solve integrates the exact trace only "
                                  "(divergence='exact'); the one-probe estimate keeps solver='rk45'")
    if divergence == "exact" and epsilon is not None:
        raise ValueError("divergence='exact' takes no probe (epsilon=None): the trace is computed, not estimated")
    if divergence == "hutchinson" and epsilon is None:
        raise ValueError("divergence='hutchinson' needs the probe epsilon [B*k,9]")
    B = cvec.shape[0]
    if method == "heun":
        if solver is None:
            if steps is None:
                raise ValueError("solver='heun' needs steps= (the number of Heun steps N; NFE = 2 N)")
            solver = HeunLikelihood(net, B, k, cvec.device, int(steps), grid=grid)
        elif steps is not None and int(steps) != solver.n:
            raise RuntimeError(f"HeunLikelihood of {solver.n} steps given for steps={steps}")
        z, delta_logp = solver.run(cvec, x.float().contiguous(), eps=eps)
        nll = (global_prior_likelihood(z.double(), SIGMA_MAX) + delta_logp) / math.log(2)
        if stats is not None:
            stats["nfev"] = int(solver.last_stats["nfev"])
            stats["attempts"] = int(solver.n)
        return z.clone(), nll
    if solver is None:
        solver = ODESampler(net, B, k, cvec.device, model=model)
    elif solver.model != ODESampler.MODELS[model]:
        raise RuntimeError(f"ODESampler(model={model!r}) required for divergence={divergence!r}")
    probe = None if epsilon is None else epsilon.to(cvec.device).float().contiguous()
    z, delta_logp = solver.run_likelihood(cvec, x.float().contiguous(), probe, eps=eps, rtol=rtol, atol=atol)
    nll = (global_prior_likelihood(z, SIGMA_MAX) + delta_logp) / math.log(2)
    if stats is not None:
        stats["nfev"] = int(solver.last_stats["nfev"])
        stats["attempts"] = int(solver.last_stats["n_attempts"])
    return z, nll
