"""Float64 restatement of the fixed-step DPM-Solver++(2M) solver of the probability-flow ODE (genpose_amd.samplers.Dpm2mSampler, the
kernels' dpm2m_update_row): the second-order multistep exponential integrator in lambda = -ln sigma on the denoiser
D = x + sigma^2 score - one evaluation per step, the previous step's denoiser carried along.  The grid, the denoising step, the finish and
the closed-form Gaussian flow are heun_reference's.  Any `score(x, t)` callable; all states are returned.  A plain helper module
(imported by the tests, not collected by pytest).

    t_0 = T0 > ... > t_N = eps,   sigma_i = sigma_min (sigma_max / sigma_min)^t_i,   lambda_i = -ln sigma_i,   h_i = lambda_{i+1} - lambda_i  (> 0)
    D_i  = x_i + sigma_i^2 score(x_i, t_i)
    r_i  = (lambda_i - lambda_{i-1}) / h_i                                  (i >= 1)
    D~_i = D_0  (i = 0),   (1 + 1/(2 r_i)) D_i - (1/(2 r_i)) D_{i-1}        (i >= 1)
    x_{i+1} = (sigma_{i+1} / sigma_i) x_i - expm1(-h_i) D~_i
"""
import numpy as np

from heun_reference import EPS, grid


def coefficients(sig):
    """What the host schedule hands the kernels per step i = 0 .. N-1, float64: sigma_i^2, sigma_{i+1} / sigma_i and the weights of D_i and
    D_{i-1} already multiplied by -expm1(-h_i) (0 for D_{-1})."""
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


def dpm2m_solve(score, x0, nsteps, T0=1.0, eps=EPS, kind="geometric", rho=7.0, t32=False):
    """All states [N+1, ...] float64 (x_0 first), the loop of the module's docstring as written there.  score(x, t) -> array like x.
    t32: hand the score the time rounded to float32 (what a network evaluated on the device sees) while the grid itself stays float64."""
    t, sig, _ = grid(nsteps, T0, eps, kind, rho)
    lam = -np.log(sig)
    tt = (lambda v: float(np.float32(v))) if t32 else float
    x = np.asarray(x0, dtype=np.float64)
    xs, D_prev = [x], None
    for i in range(int(nsteps)):
        h = lam[i + 1] - lam[i]
        D = x + sig[i] ** 2 * score(x, tt(t[i]))
        if i == 0:
            Dt = D
        else:
            r = (lam[i] - lam[i - 1]) / h
            Dt = (1.0 + 1.0 / (2.0 * r)) * D - (1.0 / (2.0 * r)) * D_prev
        x = (sig[i + 1] / sig[i]) * x - np.expm1(-h) * Dt
        D_prev = D
        xs.append(x)
    return np.stack(xs)


def dpm2m_solve_rounded(score, x0, nsteps, T0=1.0, eps=EPS, kind="geometric", rho=7.0, dtype=np.float32):
    """The device's order of operations (dpm2m_update_row) on the host schedule's coefficients, every operation rounded to `dtype`: the
    last state only.  score(x, t) must return `dtype`."""
    t, sig, _ = grid(nsteps, T0, eps, kind, rho)
    s2, ratio, wc, wp = (c.astype(dtype) for c in coefficients(sig))
    x = np.asarray(x0).astype(dtype)
    D_prev = np.zeros_like(x)
    for i in range(int(nsteps)):
        D = x + s2[i] * score(x, t[i])
        x = ratio[i] * x + (wc[i] * D + wp[i] * D_prev)
        D_prev = D
        assert x.dtype == dtype
    return x
