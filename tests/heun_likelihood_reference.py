"""Float64 restatement of the fixed-step Heun solve of the exact-likelihood ODE (genpose_amd.samplers.HeunLikelihood, the kernel
heun_likelihood_step_kernel): cond_ode_likelihood's system (networks/gf_algorithms/samplers.py:22-99) d[x; logp]/dt = -g^2/2 [score; tr J]
integrated in sigma (-g^2/2 dt = -sigma dsigma) from sigma(eps) UP to sigma(T) by Heun's method on heun_reference.grid's points in
ascending order.  Any `field(x, t) -> (score [R,9], trace [R])`.  A plain helper module (imported by the tests, not collected by pytest).

    t_0 = eps < ... < t_N = T,   sigma_i = sigma_min (sigma_max / sigma_min)^t_i,   h_i = sigma_{i+1} - sigma_i  (> 0)
    d_i = -sigma_i [score; tr](x_i, t_i);   x~ = x_i + h_i d_i[x];   d' = -sigma_{i+1} [score; tr](x~, t_{i+1})
    x_{i+1} = x_i + h_i (0.5 d_i[x] + 0.5 d'[x]);   l_{i+1} = l_i + h_i (0.5 d_i[l] + 0.5 d'[l]),  l_0 = 0
    bits = (log N(x_N; 0, sigma_max^2 I) + l_N) / ln 2
"""
import math

import numpy as np

import heun_reference as hr


def grid(nsteps, eps=hr.EPS, T=1.0, kind="geometric", rho=7.0):
    """-> (t [N+1] ascending, sigma [N+1], h [N] > 0) float64; the ends are eps and T exactly."""
    t, sig, _ = hr.grid(nsteps, T, eps, kind, rho)
    t, sig = t[::-1].copy(), sig[::-1].copy()
    return t, sig, sig[1:] - sig[:-1]


def prior_logp(z, sigma_max=hr.SIGMA_MAX):
    n = z.shape[-1]
    return -n / 2.0 * math.log(2 * math.pi * sigma_max ** 2) - np.sum(z ** 2, axis=-1) / (2 * sigma_max ** 2)


def solve(field, x0, nsteps, eps=hr.EPS, T=1.0, kind="geometric", rho=7.0):
    """-> (z [R,9], delta_logp [R], bits [R]) float64."""
    t, sig, h = grid(nsteps, eps, T, kind, rho)
    x = np.asarray(x0, dtype=np.float64)
    l = np.zeros(x.shape[0])
    for i in range(int(nsteps)):
        s, tr = field(x, float(t[i]))
        dx, dl = -sig[i] * s, -sig[i] * tr
        s2, tr2 = field(x + h[i] * dx, float(t[i + 1]))
        dx2, dl2 = -sig[i + 1] * s2, -sig[i + 1] * tr2
        x = x + h[i] * (0.5 * dx + 0.5 * dx2)
        l = l + h[i] * (0.5 * dl + 0.5 * dl2)
    return x, l, (prior_logp(x) + l) / math.log(2)


def gaussian_field(mu, s0):
    """Data N(mu, s0^2 I) diffused by the VE SDE: score = -(x - mu) / (s0^2 + sigma^2), tr J = -9 / (s0^2 + sigma^2)."""
    mu = np.asarray(mu, dtype=np.float64)

    def field(x, t):
        v = s0 * s0 + hr.sigma(t) ** 2
        return -(x - mu) / v, np.full(x.shape[0], -x.shape[1] / v)

    return field


def gaussian_truth_bits(x, mu, s0, eps=hr.EPS):
    """log N(x; mu, (s0^2 + sigma(eps)^2) I) in bits: the density of the diffused data at t = eps."""
    v = s0 * s0 + hr.sigma(eps) ** 2
    n = x.shape[1]
    return (-n / 2.0 * math.log(2 * math.pi * v) - np.sum((x - np.asarray(mu)) ** 2, axis=-1) / (2 * v)) / math.log(2)


def closed_form_field(sd, pf_rows, dtype="float64"):
    """The oracle's network as a field: exact_likelihood_ref.ClosedForm on the weights `sd` (cast to `dtype`: 'float64' the reference,
    'float32' the same closed form in the precision of the kernels) and the cloud features pf_rows [R,1024]."""
    import torch

    import exact_likelihood_ref as er
    td = torch.float64 if dtype == "float64" else torch.float32
    net = er.ClosedForm(er.f64(sd), pf_rows)
    if td is torch.float32:
        for k in ("W0", "b0", "W2", "b2", "Wa", "ba", "Wb", "bb", "Wx", "cloud"):
            setattr(net, k, getattr(net, k).float())
        net.sd = {k: (v.float() if torch.is_floating_point(v) else v) for k, v in net.sd.items()}

    def field(x, t):
        with torch.no_grad():
            xt = torch.from_numpy(np.ascontiguousarray(x)).to(td)
            if td is torch.float64:
                s, tr = net(xt, float(t))
            else:
                s, tr = _closed_form_f32(net, xt, float(t))
        return s.double().numpy(), tr.double().numpy()

    return field


def _closed_form_f32(net, x, t):
    """ClosedForm.__call__ with every tensor in float32 (its own code builds the time features in float64)."""
    import torch

    from oracle import genpose_oracle as go
    P = "pose_score_net."
    sd = net.sd
    tt = torch.tensor([t], dtype=torch.float32)
    xp = tt[:, None] * sd[P + "t_encoder.0.W"][None, :] * 2 * np.pi
    tf = torch.relu(torch.cat([torch.sin(xp), torch.cos(xp)], -1) @ sd[P + "t_encoder.1.weight"].T + sd[P + "t_encoder.1.bias"])
    h1 = torch.relu(x @ net.W0.T + net.b0)
    h2 = torch.relu(h1 @ net.W2.T + net.b2)
    a3 = torch.relu(net.cloud + tf @ net.Wa[:, 1024:1152].T + h2 @ net.Wa[:, 1152:].T)
    a3h = a3.reshape(-1, 3, 256)
    f = torch.einsum("rhc,hic->rhi", a3h, net.Wb).reshape(-1, 9) + net.bb
    g3 = (a3h > 0)[:, :, None, :] * net.Wb[None]
    g2 = torch.einsum("rhic,hcp->rhip", g3, net.Wx) * (h2 > 0)[:, None, None, :]
    g1 = (g2 @ net.W2) * (h1 > 0)[:, None, None, :]
    gx = (g1 @ net.W0).reshape(-1, 9, 9)
    s = float(go.ve_sigma(torch.tensor(t, dtype=torch.float64))) + 1e-7
    return f / s, torch.diagonal(gx, dim1=1, dim2=2).sum(-1) / s
