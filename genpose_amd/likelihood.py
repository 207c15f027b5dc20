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
"""
import math

import torch

from .samplers import ODESampler
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


def cond_ode_likelihood(net, cvec, k, x, epsilon=None, eps=1e-5, rtol=1e-5, atol=1e-5, stats=None, solver=None, divergence="hutchinson"):
    """net: ScoreNetHIP; cvec [B,768] (gp_cloud_embed); x [B*k,9] poses whose likelihood is wanted; epsilon [B*k,9] the fixed
    Hutchinson probe (the reference draws it from the prior, samplers.py:39).  Returns (z [R,9] f64, log-likelihood in bits [R] f64)
    on the device.  solver: an ODESampler of the right shape and model to reuse (buffers, captured attempts).
    divergence: 'hutchinson' (default: the reference's estimator, needs epsilon) or 'exact' (the trace itself; epsilon must be None)."""
    model = solver_model(divergence)
    if divergence == "exact" and epsilon is not None:
        raise ValueError("divergence='exact' takes no probe (epsilon=None): the trace is computed, not estimated")
    if divergence == "hutchinson" and epsilon is None:
        raise ValueError("divergence='hutchinson' needs the probe epsilon [B*k,9]")
    B = cvec.shape[0]
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
