"""float64 ground truth for the exact-divergence likelihood (helper of test_gpu_exact_likelihood.py / test_exact_likelihood_host.py; CPU).

    trace_autograd   tr(d score / d x) per row from torch.autograd.functional.jacobian on oracle.genpose_oracle.score_forward with the
                     weights and inputs cast to float64 - THE ground truth of the kernel tests; also returns the Jacobians;
    score_and_trace  the same score and trace in closed form (forward pass, ReLU masks, the nine unit seeds pushed back through the
                     transposed weights, batched) - what the float64 ODE solve calls ~1e4 times; test_exact_likelihood_host.py holds it to
                     trace_autograd at 1e-12;
    solve_f64        the likelihood ODE d[x, logp]/dt = -g^2/2 [score, tr J] from eps to 1 in float64 on tests/rk45_reference.py's
                     restatement of scipy's RK45 -> z, log-likelihood in bits, attempts.
"""
import math

import numpy as np
import torch

import rk45_reference as rr
from oracle import genpose_oracle as go

HEADS = ("rot_x", "rot_y", "trans")
P = "pose_score_net."


def f64(sd):
    return {k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}


def unit_axis_poses(R, t, gen):
    """prior x sigma(t) around unit-axis rotations: rot6 = two distinct signed unit axes, translation 0, plus N(0, sigma(t)^2) noise
    (float32 rows, as the kernels take them).  Small t: rows near the data manifold; t = 1: rows far out - mixed ReLU masks."""
    ax = torch.eye(3)
    i = torch.randint(0, 3, (R,), generator=gen)
    j = (i + 1 + torch.randint(0, 2, (R,), generator=gen)) % 3
    s = torch.randint(0, 2, (R, 2), generator=gen).float() * 2 - 1
    base = torch.cat([ax[i] * s[:, :1], ax[j] * s[:, 1:], torch.zeros(R, 3)], dim=1)
    return (base + torch.randn(R, 9, generator=gen) * float(go.ve_sigma(t))).float()


def trace_autograd(sd64, pf_rows, x, t):
    """pf_rows [R,1024], x [R,9] (any dtype; cast to float64), t float -> (score [R,9], trace [R], J [R,9,9]) float64"""
    pf_rows, x = pf_rows.double(), x.double()
    R = x.shape[0]
    J = torch.zeros(R, 9, 9, dtype=torch.float64)
    for r in range(R):
        fn = lambda xr: go.score_forward(sd64, pf_rows[r:r + 1], xr[None], torch.full((1, 1), t, dtype=torch.float64))[0]
        J[r] = torch.autograd.functional.jacobian(fn, x[r])
    score = go.score_forward(sd64, pf_rows, x, torch.full((R, 1), t, dtype=torch.float64))
    return score, torch.diagonal(J, dim1=1, dim2=2).sum(-1), J


class ClosedForm:
    """score and tr(d score / d x) of the oracle's network in float64 without autograd; the cloud part of the heads' first layer is
    evaluated once per cloud row."""

    def __init__(self, sd64, pf_rows):
        g = lambda k: sd64[P + k]
        self.sd = sd64
        self.W0, self.b0, self.W2, self.b2 = g("pose_encoder.0.weight"), g("pose_encoder.0.bias"), g("pose_encoder.2.weight"), g("pose_encoder.2.bias")
        self.Wa = torch.cat([g(f"fusion_tail_{h}.0.weight") for h in HEADS], 0)  # [768,1408] = [pts 1024 | t 128 | pose 256]
        self.ba = torch.cat([g(f"fusion_tail_{h}.0.bias") for h in HEADS], 0)
        self.Wb = torch.stack([g(f"fusion_tail_{h}.2.weight") for h in HEADS], 0)  # [3,3,256]
        self.bb = torch.cat([g(f"fusion_tail_{h}.2.bias") for h in HEADS], 0)
        self.Wx = self.Wa[:, 1152:].reshape(3, 256, 256)  # per head [channel, pose feature]
        self.cloud = pf_rows.double() @ self.Wa[:, :1024].T + self.ba  # [R,768]

    def __call__(self, x, t):
        """x [R,9] float64, t float -> (score [R,9], trace [R])"""
        sd = self.sd
        tt = torch.tensor([t], dtype=torch.float64)
        xp = tt[:, None] * sd[P + "t_encoder.0.W"][None, :] * 2 * np.pi
        tf = torch.relu(torch.cat([torch.sin(xp), torch.cos(xp)], -1) @ sd[P + "t_encoder.1.weight"].T + sd[P + "t_encoder.1.bias"])
        h1 = torch.relu(x @ self.W0.T + self.b0)
        h2 = torch.relu(h1 @ self.W2.T + self.b2)
        a3 = torch.relu(self.cloud + tf @ self.Wa[:, 1024:1152].T + h2 @ self.Wa[:, 1152:].T)  # [R,768]
        a3h = a3.reshape(-1, 3, 256)
        f = torch.einsum("rhc,hic->rhi", a3h, self.Wb).reshape(-1, 9) + self.bb
        # the nine unit seeds: seed 3 h + i = row i of head h's output layer, masked, back through Wx_h, W2, W0
        g3 = (a3h > 0)[:, :, None, :] * self.Wb[None]                       # [R,3,3,256]
        g2 = torch.einsum("rhic,hcp->rhip", g3, self.Wx) * (h2 > 0)[:, None, None, :]
        g1 = (g2 @ self.W2) * (h1 > 0)[:, None, None, :]
        gx = (g1 @ self.W0).reshape(-1, 9, 9)                               # row i = e_i^T J_f
        s = float(go.ve_sigma(torch.tensor(t, dtype=torch.float64))) + 1e-7
        return f / s, torch.diagonal(gx, dim1=1, dim2=2).sum(-1) / s


def score_and_trace(sd64, pf_rows, x, t):
    return ClosedForm(sd64, pf_rows)(x.double(), float(t))


def solve_f64(sd, pf_rows, x, eps=1e-5, rtol=1e-5, atol=1e-5):
    """-> (z [R,9], log-likelihood in bits [R], attempts): the exact-divergence likelihood ODE in float64, state [x (R*9); logp (R)] as
    cond_ode_likelihood lays it out, one error norm over the whole vector."""
    R = x.shape[0]
    net = ClosedForm(f64(sd), pf_rows)

    def fun(t, y):
        xt = torch.from_numpy(np.ascontiguousarray(y[:R * 9].reshape(R, 9)))
        score, tr = net(xt, float(t))
        g2 = float(go.ve_diffusion(torch.tensor(float(t), dtype=torch.float64))) ** 2
        return np.concatenate([(-0.5 * g2) * score.numpy().reshape(-1), (-0.5 * g2) * tr.numpy()])

    y0 = np.concatenate([x.double().numpy().reshape(-1), np.zeros(R)])
    with torch.no_grad():
        log, states = rr.replay_run(fun, eps, y0, 1.0, rtol=rtol, atol=atol)
    y = states[-1]
    z = y[:R * 9].reshape(R, 9)
    smax = float(go.ve_sigma(1.0))
    prior = -9 / 2.0 * math.log(2 * math.pi * smax ** 2) - (z ** 2).sum(-1) / (2 * smax ** 2)
    return z, (prior + y[R * 9:]) / math.log(2), len(log)
