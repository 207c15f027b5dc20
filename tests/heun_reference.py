"""Float64 restatement of the fixed-step Heun solver of the probability-flow ODE (genpose_amd.samplers.HeunSampler, the kernels'
heun_update_row): Heun's second-order method on a sigma grid - cond_edm_sampler's loop (networks/gf_algorithms/samplers.py:230-290) -
driven by a VE score through denoised = x + sigma^2 score, i.e. with the slope d = -sigma score.  Any `score(x, t)` callable; all states
are returned.  A plain helper module (imported by the tests, not collected by pytest).

    t_0 = T0 > ... > t_N = eps,   sigma_i = sigma_min (sigma_max / sigma_min)^t_i,   h_i = sigma_{i+1} - sigma_i  (< 0)
    d_i = -sigma_i score(x_i, t_i);   x~ = x_i + h_i d_i;   d' = -sigma_{i+1} score(x~, t_{i+1});   x_{i+1} = x_i + h_i (0.5 d_i + 0.5 d')
"""
import math

import numpy as np

SIGMA_MIN, SIGMA_MAX, EPS = 0.01, 50.0, 1e-5
RATIO = SIGMA_MAX / SIGMA_MIN
G_FACTOR = math.sqrt(2.0 * (math.log(SIGMA_MAX) - math.log(SIGMA_MIN)))  # g(t) = sigma(t) * G_FACTOR


def sigma(t):
    return SIGMA_MIN * RATIO ** t


def grid(nsteps, T0=1.0, eps=EPS, kind="geometric", rho=7.0):
    """-> (t [N+1], sigma [N+1], h [N]) float64.  'geometric': t uniform; 'edm': the rho discretisation of cond_edm_sampler
    (samplers.py:241-242) between sigma(T0) and sigma(eps), mapped back to t.  The ends are T0 and eps exactly."""
    N = int(nsteps)
    if kind == "geometric":
        t = np.linspace(float(T0), float(eps), N + 1)
    elif kind == "edm":
        s_hi, s_lo = SIGMA_MIN * RATIO ** float(T0), SIGMA_MIN * RATIO ** float(eps)
        idx = np.arange(N + 1, dtype=np.float64)
        s = (s_hi ** (1.0 / rho) + idx / N * (s_lo ** (1.0 / rho) - s_hi ** (1.0 / rho))) ** rho
        t = np.log(s / SIGMA_MIN) / np.log(RATIO)
    else:
        raise ValueError(kind)
    t[0], t[-1] = float(T0), float(eps)
    sig = SIGMA_MIN * RATIO ** t
    return t, sig, sig[1:] - sig[:-1]


def heun_solve(score, x0, nsteps, T0=1.0, eps=EPS, kind="geometric", rho=7.0, t32=False):
    """All states [N+1, ...] float64 (x_0 first).  score(x, t) -> array like x.  t32: hand the score the time rounded to float32 (what a
    network evaluated on the device sees) while the grid itself stays float64."""
    t, sig, h = grid(nsteps, T0, eps, kind, rho)
    tt = (lambda v: float(np.float32(v))) if t32 else float
    x = np.asarray(x0, dtype=np.float64)
    xs = [x]
    for i in range(int(nsteps)):
        d = -sig[i] * score(x, tt(t[i]))
        xe = x + h[i] * d
        dp = -sig[i + 1] * score(xe, tt(t[i + 1]))
        x = x + h[i] * (0.5 * d + 0.5 * dp)
        xs.append(x)
    return np.stack(xs)


def denoise(score, x, nsteps, eps=EPS, t32=False):
    """The reverse-diffusion predictor at eps of cond_ode_sampler (samplers.py:209-218) with its divisor rule for num_steps = N:
    x + (0 - g(eps)^2 score(x, eps)) (1 - eps) / N."""
    te = float(np.float32(eps)) if t32 else float(eps)
    g = sigma(float(eps)) * G_FACTOR
    return x + (0.0 - g * g * score(x, te)) * ((1.0 - float(eps)) / int(nsteps))


def normalize_rot6(x):
    """normalize_rotation for pose_mode 'rot_matrix' (utils/misc.py:259-265): Gram-Schmidt of the two columns; x [..., 9]."""
    x = np.array(x, dtype=np.float64)
    a1, a2 = x[..., 0:3], x[..., 3:6]
    b1 = a1 / np.maximum(np.linalg.norm(a1, axis=-1, keepdims=True), 1e-12)
    b2 = a2 - np.sum(b1 * a2, axis=-1, keepdims=True) * b1
    b2 = b2 / np.maximum(np.linalg.norm(b2, axis=-1, keepdims=True), 1e-12)
    x[..., 0:3], x[..., 3:6] = b1, b2
    return x


def finish(x, centre_rows):
    """normalize_rotation, then the cloud centre added to the translation (samplers.py:220-226); centre_rows broadcasts against x[..., 6:]."""
    y = normalize_rot6(x)
    y[..., 6:9] += centre_rows
    return y


def gaussian_score(s):
    """VE score of the data distribution N(0, s^2 I): -x / (s^2 + sigma(t)^2).  Its flow: x(sigma) = x(sigma_0) sqrt((s^2 + sigma^2) / (s^2 + sigma_0^2))."""
    return lambda x, t: -x / (s * s + sigma(t) ** 2)


def gaussian_flow(x0, s, T0, t):
    return x0 * math.sqrt((s * s + sigma(t) ** 2) / (s * s + sigma(T0) ** 2))
