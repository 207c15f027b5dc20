"""Float64 ground truth for the device RK45 solver (csrc/rk45.hip): analytic-field networks, their exact solutions, one
Dormand-Prince attempt and scipy's step controller written out on scipy's own step code, and a test-side driver that runs an
ODESampler up to the raw accepted states.  A plain helper module (imported by the tests, not collected by pytest).

Analytic field: a state dict in the reference layout whose trunk computes the affine map

    f_theta(x, t, cloud) = A x + c_cloud + d tau(t),     c_cloud = Cw . pts_feat[chans] + bias,   tau(t) = sin(2 pi omega t) + 2

exactly: the pose encoder maps x to [x+; x-] (ReLU of +x and -x), identity layers and ReLUs pass those (and the encoder features,
which are >= 0 after the encoder's last ReLU and max-pool) through unchanged, and the head output layers compute A (x+ - x-) + ...
Every model of the driver then has a right-hand side in closed form (score / energy / likelihood below)."""
import math

import numpy as np
import scipy.integrate
import scipy.linalg
from scipy.integrate._ivp import rk as _rk
from scipy.integrate._ivp.rk import RK45

SIGMA_MIN, SIGMA_MAX, EPS = 0.01, 50.0, 1e-5
LOG_RATIO = math.log(SIGMA_MAX) - math.log(SIGMA_MIN)
U32 = 2.0 ** -24  # unit roundoff of float32
U64 = 2.0 ** -53

# Dormand-Prince tableau and scipy's controller constants, taken from scipy itself
DP_A, DP_B, DP_C, DP_E, DP_P = RK45.A, RK45.B, RK45.C, RK45.E, RK45.P
SAFETY, MIN_FACTOR, MAX_FACTOR = _rk.SAFETY, _rk.MIN_FACTOR, _rk.MAX_FACTOR
ERR_EXP = -1.0 / (RK45.error_estimator_order + 1)

# hidden-unit layout of every head of the analytic network
_POSE_IN, _TIME_IN = 1152, 1024  # offsets of pose_feat / t_feat in the trunk's concatenated input [pts 1024 | t 128 | pose 256]


def sigma(t):
    return SIGMA_MIN * (SIGMA_MAX / SIGMA_MIN) ** t


def g2(t):
    return sigma(t) ** 2 * 2.0 * LOG_RATIO


def a_score(t):
    """dx/dt = a(t) f_theta of the probability-flow ODE (score = f / (sigma + 1e-7))."""
    return -0.5 * g2(t) / (sigma(t) + 1e-7)


def a_energy(t):
    """the energy model divides by sigma itself (energynet.py)."""
    return -0.5 * g2(t) / sigma(t)


class AnalyticNet:
    """A [9,9]; Cw [9,nf] weights of the encoder-feature channels `chans`; bias [9]; d [9] (time term) or None; omega."""

    def __init__(self, A, Cw, chans, bias=None, d=None, omega=0.2):
        self.A = np.asarray(A, dtype=np.float64)
        self.Cw = np.asarray(Cw, dtype=np.float64)
        self.chans = list(chans)
        self.bias = np.zeros(9) if bias is None else np.asarray(bias, dtype=np.float64)
        self.d = None if d is None else np.asarray(d, dtype=np.float64)
        self.omega = float(omega)
        # the network computes in float32: the field is the one of the float32-rounded weights
        for name in ("A", "Cw", "bias", "d"):
            v = getattr(self, name)
            if v is not None:
                setattr(self, name, v.astype(np.float32).astype(np.float64))
        self.omega = float(np.float32(self.omega))

    def state_dict(self, template):
        return analytic_state_dict(self, template)

    def tau(self, t):
        return np.sin(2 * np.pi * self.omega * np.asarray(t, dtype=np.float64)) + 2.0

    def offsets(self, pts_feat):
        """c per cloud [B,9] from encoder features [B,1024] (float64 of the float32 features)."""
        pf = np.asarray(pts_feat, dtype=np.float64)
        return pf[:, self.chans] @ self.Cw.T + self.bias

    def f_theta(self, t, x, c_rows):
        """x, c_rows [R,9] -> A x + c + d tau(t)"""
        f = x @ self.A.T + c_rows
        if self.d is not None:
            f = f + self.d * self.tau(t)
        return f

    def magnitude(self, t, x, c_rows):
        """sum of |terms| the float32 layer sums add per component: the scale of their rounding error"""
        m = np.abs(x) @ np.abs(self.A).T + np.abs(c_rows) + 0.0
        if self.d is not None:
            m = m + np.abs(self.d) * 3.0
        return m


def analytic_state_dict(net, template):
    """Reference-layout state dict (same keys and shapes as `template`, e.g. genpose_oracle.make_state_dict(0, 'score')) of the
    analytic field of `net`.  The encoder weights are kept (they only produce pts_feat)."""
    import torch
    sd = {k: v.clone() for k, v in template.items()}
    q = "pose_score_net."
    z = lambda k: torch.zeros_like(sd[q + k])
    nf = len(net.chans)
    if 18 + nf + 1 > 256:
        raise ValueError("too many feature channels")
    w = z("pose_encoder.0.weight")  # [256, 9]
    for i in range(9):
        w[i, i], w[9 + i, i] = 1.0, -1.0
    sd[q + "pose_encoder.0.weight"], sd[q + "pose_encoder.0.bias"] = w, z("pose_encoder.0.bias")
    w = z("pose_encoder.2.weight")
    for i in range(18):
        w[i, i] = 1.0
    sd[q + "pose_encoder.2.weight"], sd[q + "pose_encoder.2.bias"] = w, z("pose_encoder.2.bias")
    W = z("t_encoder.0.W")
    W[0] = net.omega
    sd[q + "t_encoder.0.W"] = W
    w, b = z("t_encoder.1.weight"), z("t_encoder.1.bias")
    w[0, 0], b[0] = 1.0, 2.0  # t_feat[0] = relu(sin(2 pi omega t) + 2) = tau(t)
    sd[q + "t_encoder.1.weight"], sd[q + "t_encoder.1.bias"] = w, b
    tunit = 18 + nf
    for h, head in enumerate(("rot_x", "rot_y", "trans")):
        p = f"fusion_tail_{head}"
        w0 = z(p + ".0.weight")  # [256, 1408]
        for i in range(18):
            w0[i, _POSE_IN + i] = 1.0
        for j, ch in enumerate(net.chans):
            w0[18 + j, ch] = 1.0
        w0[tunit, _TIME_IN] = 1.0
        sd[q + p + ".0.weight"], sd[q + p + ".0.bias"] = w0, z(p + ".0.bias")
        w2 = z(p + ".2.weight")  # [3, 256]
        rows = slice(3 * h, 3 * h + 3)
        w2[:, 0:9] = torch.from_numpy(net.A[rows]).float()
        w2[:, 9:18] = -torch.from_numpy(net.A[rows]).float()
        w2[:, 18:18 + nf] = torch.from_numpy(net.Cw[rows]).float()
        if net.d is not None:
            w2[:, tunit] = torch.from_numpy(net.d[rows]).float()
        sd[q + p + ".2.weight"], sd[q + p + ".2.bias"] = w2, torch.from_numpy(net.bias[rows]).float()
    return sd


# ----------------------------------------------------------------------------- the problems the tests use
CHANS = [3, 100, 517, 900]  # encoder-feature channels that carry the per-cloud offsets


def problems():
    """name -> (AnalyticNet, driver model).  Non-stiff, contracting in the direction of integration (t decreasing for the samplers,
    increasing for the likelihood: A with a positive symmetric part, since a(t) < 0); 'time' has a fast time-only forcing term
    and rejected attempts."""
    rng = np.random.default_rng(0)
    S = rng.standard_normal((9, 9))
    S = (S - S.T) / 2
    Cw = rng.standard_normal((9, len(CHANS))) * 0.5
    d = rng.standard_normal(9) * 20
    rng = np.random.default_rng(2)
    S2 = rng.standard_normal((9, 9))
    S2 = (S2 - S2.T) / 2
    return {
        "contract": (AnalyticNet(-0.08 * np.eye(9) + 0.03 * S, Cw, CHANS), "score"),
        "time": (AnalyticNet(-0.08 * np.eye(9) + 0.03 * S, Cw, CHANS, d=d, omega=3.0), "score"),
        "energy": (AnalyticNet(-0.04 * np.eye(9) + 0.03 * S, Cw, CHANS), "energy"),
        "likelihood": (AnalyticNet(0.02 * np.eye(9) + 0.01 * S2, rng.standard_normal((9, len(CHANS))) * 0.5, CHANS), "likelihood"),
    }


def inputs(B, K, T0, seed=0, likelihood=False):
    """pts_feat [B,1024] (>= 0, like the encoder's output), initial rows [B*K,9] float32 (prior draws x sigma(T0); standard normal
    for the likelihood) and a Hutchinson probe [B*K,9] float32"""
    rng = np.random.default_rng(100 + seed)
    pf = np.abs(rng.standard_normal((B, 1024))).astype(np.float32)
    x = rng.standard_normal((B * K, 9))
    x = (x if likelihood else x * sigma(T0)).astype(np.float32)
    probe = rng.standard_normal((B * K, 9)).astype(np.float32)
    return pf, x, probe


# ----------------------------------------------------------------------------- float64 right-hand sides (from the definitions)
class Field:
    """Right-hand side of one driver model on the analytic network, float64.  Rows carry their own cloud offset c_rows [R,9];
    the likelihood model also a probe [R,9].  __call__(t, Y [R,nc]) -> dY/dt [R,nc]; bound(t, Y) -> componentwise bound on
    |device float32 evaluation - this| (network sums in float32, float32 sigma, float32 network input)."""

    def __init__(self, net, model, c_rows, probe=None):
        self.net, self.model, self.c = net, model, np.asarray(c_rows, dtype=np.float64)
        self.probe = None if probe is None else np.asarray(probe, dtype=np.float64)
        self.nc = 10 if model == "likelihood" else 9
        self.nfev = 0

    def __call__(self, t, Y):
        self.nfev += 1
        net, x = self.net, Y[:, :9]
        if self.model == "score":
            return a_score(t) * net.f_theta(t, x, self.c)
        if self.model == "energy":
            return a_energy(t) * (net.f_theta(t, x, self.c) + x @ net.A)  # ((A + A^T) x + c + d tau) / sigma
        out = np.empty_like(Y)
        out[:, :9] = a_score(t) * net.f_theta(t, x, self.c)
        out[:, 9] = a_score(t) * np.einsum("ri,ij,rj->r", self.probe, net.A, self.probe)
        return out

    def bound(self, t, Y):
        net, x = self.net, Y[:, :9]
        m = net.magnitude(t, x, self.c)
        if self.model == "energy":
            m = m + np.abs(x) @ np.abs(net.A)
        # 32 u of the summed magnitudes: the output layer's float32 sum (at most 9 + nf + 2 nonzero terms), the float32 input,
        # sigma in float32 (powf of a float32 t: |d ln sigma / dt| t u < 9 u) and the divisions
        b = np.empty_like(Y)
        a = abs(a_energy(t) if self.model == "energy" else a_score(t))
        b[:, :9] = 32 * U32 * a * m
        if self.model == "likelihood":
            pm = np.einsum("ri,ij,rj->r", np.abs(self.probe), np.abs(net.A), np.abs(self.probe))
            b[:, 9] = 32 * U32 * a * pm
        return b


def fun_flat(field, R):
    """solve_ivp / RK45 form of a Field (flat float64 vector)"""
    return lambda t, y: field(t, y.reshape(R, field.nc)).reshape(-1)


# ----------------------------------------------------------------------------- exact solutions
def phi(a_fn, t0, t1):
    """U = int_t0^t1 a(s) ds"""
    v, _ = scipy.integrate.quad(a_fn, t0, t1, epsabs=0.0, epsrel=1.2e-14, limit=200)
    return v


def _prop(Aeff, U):
    """expm(Aeff U) and int_0^U expm(Aeff s) ds (one augmented exponential)"""
    M = np.zeros((18, 18))
    M[:9, :9], M[:9, 9:] = Aeff * U, np.eye(9) * U
    E = scipy.linalg.expm(M)
    return E[:9, :9], E[:9, 9:]


def exact_solution(net, model, x0, c_rows, t0, ts):
    """x(t) for every t in ts of dx/dt = a(t) (Aeff x + c + d tau(t)), x(t0) = x0 [R,9] -> [len(ts), R, 9].
    Closed form (quadrature + expm) for the time-independent part; the time term is row independent and comes from one
    9-dimensional DOP853 solve at rtol 1e-13."""
    a_fn = a_energy if model == "energy" else a_score
    Aeff = net.A + net.A.T if model == "energy" else net.A
    x0, c = np.asarray(x0, dtype=np.float64), np.asarray(c_rows, dtype=np.float64)
    out = []
    w_at = None
    if net.d is not None:
        w_at = {float(t0): np.zeros(9)}
        pts = np.unique([float(t) for t in ts if float(t) != float(t0)])
        if pts.size:
            te = pts if pts[0] > t0 else pts[::-1]  # t_eval in the direction of integration (all points lie on one side of t0)
            rhs = lambda t, w: a_fn(t) * (Aeff @ w + net.d * net.tau(t))
            sol = scipy.integrate.solve_ivp(rhs, (t0, float(te[-1])), np.zeros(9), method="DOP853", rtol=1e-13, atol=1e-14, t_eval=te)
            assert sol.success
            for k, tt in enumerate(te):
                w_at[float(tt)] = sol.y[:, k]
    for t in ts:
        U = phi(a_fn, t0, float(t))
        E, F = _prop(Aeff, U)
        x = x0 @ E.T + c @ F.T
        if w_at is not None:
            x = x + w_at[float(t)]
        out.append(x)
    return np.stack(out)



def dop853_solution(field, Y0, t0, t1):
    """the same ODE by solve_ivp(DOP853, rtol 1e-13) on the whole state (cross-check of exact_solution)"""
    R = Y0.shape[0]
    sol = scipy.integrate.solve_ivp(fun_flat(field, R), (t0, t1), Y0.reshape(-1), method="DOP853", rtol=1e-13, atol=1e-12)
    return sol.y[:, -1].reshape(R, -1)


def exact_likelihood(net, x, probe, c_rows, eps=EPS):
    """closed form of cond_ode_likelihood on the analytic field: z = x(1), delta_logp = eps^T A eps . int_eps^1 a, bits"""
    z = exact_solution(net, "score", x, c_rows, eps, [1.0])[0]
    dlogp = np.einsum("ri,ij,rj->r", probe, net.A, probe) * phi(a_score, eps, 1.0)
    prior = -9 / 2.0 * math.log(2 * math.pi * SIGMA_MAX ** 2) - np.sum(z ** 2, axis=-1) / (2 * SIGMA_MAX ** 2)
    return z, dlogp, (prior + dlogp) / math.log(2)


# ----------------------------------------------------------------------------- one attempt and the controller (scipy's step code)
def rms(x):
    return np.linalg.norm(x) / x.size ** 0.5


def dp_attempt(fun, t, y, f0, h, rtol, atol):
    """one Dormand-Prince attempt from (t, y) with signed step h on scipy's rk_step -> (y_new, f_new, K [7,n], err_norm, stage_y [7,n])"""
    n = y.size
    K = np.empty((7, n))
    stage_y = np.empty((7, n))
    stage_y[0] = y
    calls = []

    def rec(tt, yy):
        calls.append(yy.copy())
        return fun(tt, yy)

    y_new, f_new = _rk.rk_step(rec, t, y, f0, h, DP_A, DP_B, DP_C, K)
    for s in range(1, 6):
        stage_y[s] = calls[s - 1]
    stage_y[6] = y_new
    scale = atol + np.maximum(np.abs(y), np.abs(y_new)) * rtol
    err = rms(K.T.dot(DP_E) * h / scale)
    return y_new, f_new, K, err, stage_y


def next_h_abs(h_abs, err, step_rejected):
    """scipy's _step_impl update of |h| after an attempt with error norm err"""
    if err < 1:
        factor = MAX_FACTOR if err == 0 else min(MAX_FACTOR, SAFETY * err ** ERR_EXP)
        if step_rejected:
            factor = min(1, factor)
        return h_abs * factor
    return h_abs * max(MIN_FACTOR, SAFETY * err ** ERR_EXP)


def clip_step(t, h_abs, direction, t_bound, step_rejected):
    """start of an attempt (rk.py _step_impl): min_step rule and the t_bound clip -> (signed h, t_new) or None (too small)"""
    min_step = 10 * np.abs(np.nextafter(t, direction * np.inf) - t)
    if h_abs < min_step:
        if step_rejected:
            return None
        h_abs = min_step
    h = h_abs * direction
    t_new = t + h
    if direction * (t_new - t_bound) > 0:
        t_new = t_bound
    return t_new - t, t_new


def initial_step(t0, y0, f0, f1_fun, t_bound, rtol, atol):
    """scipy's select_initial_step (order 4) -> (h0, h_abs of the first attempt, d0, d1, d2)"""
    interval = abs(t_bound - t0)
    direction = np.sign(t_bound - t0)
    scale = atol + np.abs(y0) * rtol
    d0, d1 = rms(y0 / scale), rms(f0 / scale)
    h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
    h0 = min(h0, interval)
    f1 = f1_fun(t0 + h0 * direction, y0 + h0 * direction * f0)
    d2 = rms((f1 - f0) / scale) / h0
    h1 = max(1e-6, h0 * 1e-3) if (d1 <= 1e-15 and d2 <= 1e-15) else (0.01 / max(d1, d2)) ** 0.2
    return h0, min(100 * h0, h1, interval), d0, d1, d2


def replay_run(fun, t0, y0, t_bound, rtol=1e-5, atol=1e-5, max_attempts=100000):
    """the whole adaptive solve on dp_attempt + next_h_abs + clip_step -> list of attempts (t, h, err, acc) and accepted states"""
    direction = np.sign(t_bound - t0)
    y = np.asarray(y0, dtype=np.float64).copy()
    t = t0
    f = fun(t, y)
    _, h_abs, *_ = initial_step(t0, y, f, fun, t_bound, rtol, atol)
    log, states = [], [y.copy()]
    while direction * (t - t_bound) < 0 and len(log) < max_attempts:
        rejected = False
        while True:
            r = clip_step(t, h_abs, direction, t_bound, rejected)
            if r is None:
                raise RuntimeError("step size too small")
            h, t_new = r
            y_new, f_new, _, err, _ = dp_attempt(fun, t, y, f, h, rtol, atol)
            log.append(dict(t=t, h=h, err=err, acc=bool(err < 1)))
            h_abs = next_h_abs(abs(h), err, rejected)
            if err < 1:
                break
            rejected = True
        t, y, f = t_new, y_new, f_new
        states.append(y.copy())
    return log, states


def scipy_run(fun, t0, y0, t_bound, rtol=1e-5, atol=1e-5):
    """scipy.integrate.RK45 itself, every evaluation time recorded -> (nfev, accept sequence, attempt start times, attempt steps,
    accepted states).  An attempt is six evaluations (after the two of the initial step); after a rejection the next attempt
    starts from the same t."""
    times = []

    def rec(t, y):
        times.append(t)
        return fun(t, y)

    errs = []

    class Recorded(RK45):
        def _estimate_error_norm(self, K, h, scale):
            e = super()._estimate_error_norm(K, h, scale)
            errs.append(e)
            return e

    s = Recorded(rec, t0, np.asarray(y0, dtype=np.float64), t_bound, rtol=rtol, atol=atol)
    states, ts = [s.y.copy()], [s.t]
    while s.status == "running":
        msg = s.step()
        if s.status == "failed":
            raise RuntimeError(msg)
        states.append(s.y.copy())
        ts.append(s.t)
    ev = np.asarray(times)
    # evaluation 0 = f(t0) (RK45.__init__), 1 = the initial-step probe; attempt i = evaluations 2 + 6 i .. 7 + 6 i
    n_att = (len(ev) - 2) // 6
    assert len(ev) == 2 + 6 * n_att
    direction = np.sign(t_bound - t0)
    starts, hs, acc = [], [], []
    t_cur = t0
    for i in range(n_att):
        t_end = ev[7 + 6 * i]  # the sixth evaluation of an attempt is at t_new = t + h
        starts.append(t_cur)
        hs.append(t_end - t_cur)
        # accepted <=> the next attempt starts at t_new: its first stage time t_new + c1 h' lies beyond t_new
        accepted = True if i + 1 == n_att else bool(direction * (ev[2 + 6 * (i + 1)] - t_end) > 0)
        acc.append(accepted)
        if accepted:
            t_cur = t_end
    return dict(nfev=len(ev), acc=np.asarray(acc), err=np.asarray(errs), t=np.asarray(starts), h=np.asarray(hs), states=states, ts=np.asarray(ts))


def err_noise(field, t, y, h, stage_y, rtol=1e-5, atol=1e-5, y_new=None):
    """absolute bound on |device err_norm - float64 err_norm| of one attempt: the float32 evaluation bound of every stage through
    h |E_j| (the error estimate is linear in the stage derivatives), plus the stage-state perturbation it causes"""
    R = y.size // field.nc
    yn = stage_y[6] if y_new is None else y_new
    scale = atol + np.maximum(np.abs(y), np.abs(yn)) * rtol
    tot = np.zeros(y.size)
    for j in range(7):
        tj = t + DP_C[j] * h if j < 6 else t + h
        tot += abs(DP_E[j]) * field.bound(tj, stage_y[j].reshape(R, field.nc)).reshape(-1)
    return 2.0 * rms(np.abs(h) * tot / scale) + 1e-12


def step_bound(field, t, h, stage_y):
    """componentwise bound on |device y_new - float64 y_new| from (t, y, h): sum_j |h b_j| x the float32 bound of stage j, twice
    for the propagation of a stage's error through the later stage states (|h A| stays well inside the stability region)"""
    R = stage_y.shape[1] // field.nc
    tot = np.zeros(stage_y.shape[1])
    for j in range(6):
        tot += abs(DP_B[j]) * field.bound(t + DP_C[j] * h, stage_y[j].reshape(R, field.nc)).reshape(-1)
    return 2.0 * abs(h) * tot + 1e-13


# ----------------------------------------------------------------------------- test-side device driver
def solve_raw(smp, cvec, y0, t0, t_bound, rtol=1e-5, atol=1e-5, probe=None, max_attempts=4096):
    """Runs an ODESampler the way run() / run_likelihood() do - phases 0-2 and the adaptive loop (_solve, with graphs when the
    sampler uses them) - recording every accepted state in a trajectory buffer, and WITHOUT phases 4-5, so the states stay raw
    (no denoise, normalisation or centre).  y0 [R, nc] float64 (device).  Returns per group: dict(log_t, log_h, log_err, log_acc,
    n_attempts, n_accepted, nfev, states [n_accepted + 1, rows of the group, nc] float64 numpy)."""
    import torch
    R, nc = smp.R, smp.ncomp
    smp.cvec[: cvec.shape[0]].copy_(cvec)
    smp.centre.zero_()
    if probe is not None:
        smp.probe.copy_(probe.float())
    smp.y[: y0.numel()].copy_(y0.reshape(-1).double())
    traj = getattr(smp, "_raw_traj", None)
    if traj is None:
        traj = smp._raw_traj = torch.zeros(smp.TRAJ_CAP, R * nc, dtype=torch.float64, device=smp.dev)
    smp._phase(0, traj, t0=t0, t_bound=t_bound, rtol=rtol, atol=atol)
    smp._phase(1, traj)
    smp._phase(2, traj)
    sts = smp._solve(traj, "graph_raw", t0, max_attempts)
    tr = traj.cpu().numpy().reshape(smp.TRAJ_CAP, R, nc)
    out = []
    if smp.ragged:
        bounds, r0 = [], 0
        for c in smp.group_clouds:
            bounds.append((r0, r0 + c * smp.K))
            r0 += c * smp.K
    else:
        rg = R // smp.groups
        bounds = [(g * rg, (g + 1) * rg) for g in range(smp.groups)]
    for st, (lo, hi) in zip(sts, bounds):
        na = int(st["n_accepted"])
        if na + 1 > smp.TRAJ_CAP:
            raise RuntimeError("trajectory capacity exceeded")
        d = dict(st)
        d["states"] = tr[: na + 1, lo:hi].copy()
        out.append(d)
    return out


def replay_check(field, run, t0, t_bound, rtol=1e-5, atol=1e-5):
    """Replays every logged attempt of one device solve (a solve_raw group) in float64 from the device's own state and step (the
    first 512 attempts of a longer solve: the device's log holds no more).  Raises AssertionError with the attempt index on a violation; returns the largest discrepancy of each kind as a fraction of
    its bound."""
    states, lt, lh, le, la = run["states"], run["log_t"], run["log_h"], run["log_err"], run["log_acc"]
    n_all = int(run["n_attempts"])
    n_att = min(n_all, 512)  # the device logs its first 512 attempts (Rk45State::log_*): a longer solve is replayed up to there
    assert len(lt) == len(lh) == len(le) == len(la) == n_att
    assert int(run["nfev"]) == 2 + 6 * n_all, f"nfev {run['nfev']} != 2 + 6 x {n_all}"
    rows = states.shape[1]
    direction = np.sign(t_bound - t0)
    fun = lambda t, y: field(t, y.reshape(rows, field.nc)).reshape(-1)
    worst = dict(state=0.0, err=0.0, h=0.0, h0=0.0)
    # initial step from the device's y0 (float64 field: d1 / d2 carry the float32 noise of f0 / f1)
    y = states[0].reshape(-1)
    f0 = fun(t0, y)
    h0, h_abs, d0, d1, d2 = initial_step(t0, y, f0, fun, t_bound, rtol, atol)
    scale = atol + np.abs(y) * rtol
    b0 = field.bound(t0, y.reshape(rows, field.nc)).reshape(-1)
    rel_d1 = 4 * rms(b0 / scale) / d1
    y1 = y + h0 * direction * f0
    b1 = field.bound(t0 + h0 * direction, y1.reshape(rows, field.nc)).reshape(-1)
    abs_d2 = 4 * (rms(b0 / scale) + rms(b1 / scale)) / h0
    tol_h0 = (rel_d1 + 0.2 * (rel_d1 + abs_d2 / max(d1, d2)) + 1e-13) * h_abs
    got0 = abs(lh[0])
    worst["h0"] = abs(got0 - h_abs) / tol_h0
    assert abs(got0 - h_abs) <= tol_h0 or (abs(h_abs - abs(t_bound - t0)) < 1e-15 and got0 == abs(t_bound - t0)), \
        f"initial step {got0!r} vs {h_abs!r} (tol {tol_h0:.2e})"
    assert lt[0] == t0
    k = 0  # accepted states so far
    rejected = False
    f = f0
    for i in range(n_att):
        t, h, err_dev, acc = float(lt[i]), float(lh[i]), float(le[i]), bool(la[i])
        y = states[k].reshape(-1)
        if i > 0:
            f = fun(t, y)
        y_new, _, _, err_ref, stage_y = dp_attempt(fun, t, y, f, h, rtol, atol)
        assert acc == (err_dev < 1.0), f"attempt {i}: acc flag {acc} with err_norm {err_dev}"
        tol_e = err_noise(field, t, y, h, stage_y, rtol, atol)
        worst["err"] = max(worst["err"], abs(err_dev - err_ref) / tol_e)
        assert abs(err_dev - err_ref) <= tol_e, f"attempt {i}: err_norm {err_dev!r} vs float64 {err_ref!r} (tol {tol_e:.2e})"
        if abs(err_ref - 1.0) > tol_e:
            assert acc == (err_ref < 1.0), f"attempt {i}: decision differs from float64 outside the noise band"
        if acc:
            k += 1
            got = states[k].reshape(-1)
            tol_y = step_bound(field, t, h, stage_y)
            ratio = np.max(np.abs(got - y_new) / tol_y)
            worst["state"] = max(worst["state"], ratio)
            assert ratio <= 1.0, f"attempt {i} (t={t}, h={h}): accepted state off by {ratio:.2f} x its bound"
        # controller: the next attempt follows from the device's own err_norm
        h_abs_next = next_h_abs(abs(h), err_dev, rejected)
        rejected = not acc
        if i + 1 < n_att:
            r = clip_step(float(lt[i + 1]), h_abs_next, direction, t_bound, rejected)
            assert r is not None
            h_pred = r[0]
            if acc:
                # (the device keeps t_new itself, which t + h with h = t_new - t may miss by an ulp)
                assert abs(lt[i + 1] - (t + h)) <= 2 * U64 * abs(t + h), f"attempt {i + 1} starts at {lt[i + 1]!r}, expected {t + h!r}"
            else:
                assert lt[i + 1] == t, f"attempt {i + 1} after a rejection starts at {lt[i + 1]!r}, expected {t!r}"
            dh = abs(float(lh[i + 1]) - h_pred) / (4 * U64 * abs(h_pred) + 4 * U64 * abs(float(lt[i + 1])))
            worst["h"] = max(worst["h"], dh)
            assert dh <= 1.0, f"attempt {i + 1}: h {lh[i + 1]!r} vs controller {h_pred!r}"
        elif n_att == n_all:
            assert acc and direction * (t + h - t_bound) >= 0 - 1e-15, "the last attempt must be accepted and reach t_bound"
    if n_att == n_all:
        assert k == int(run["n_accepted"]) == states.shape[0] - 1
    else:
        assert k <= int(run["n_accepted"]) == states.shape[0] - 1
    return worst


# ----------------------------------------------------------------------------- arbitrary weights (seeded random, trained checkpoints)
class NetField:
    """Probability-flow right-hand side of the score network with ANY reference-layout weights, in float64 through the oracle's
    trunk (genpose_oracle._trunk on a float64 copy of the state dict).  pts_feat [B,1024]: the encoder features the device used
    (float32 values, exact in float64); rows are cloud-major, K per cloud.

    bound(): componentwise bound on |device float32 evaluation - this|, propagated through the trunk layer by layer in float64
    (value and error bound side by side): a float32 sum of n products is taken to be within 4 sqrt(n) u of the summed magnitudes
    (the probabilistic rounding-error bound: independent roundings add like a random walk; the worst case n u is never approached
    by a 1408-term sum), an error already in a layer's input passes through |W|, ReLU does not expand it."""

    def __init__(self, sd, pts_feat, K):
        import torch
        self.sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        self.feat = torch.as_tensor(np.asarray(pts_feat, dtype=np.float64)).repeat_interleave(K, 0)
        self.model, self.nc, self.nfev = "score", 9, 0

    def _net(self, t, x):
        import torch
        from oracle import genpose_oracle as go
        R = x.shape[0]
        return go._trunk(self.sd, self.feat[:R], torch.as_tensor(x), torch.full((R, 1), float(t), dtype=torch.float64)).numpy()

    def __call__(self, t, Y):
        self.nfev += 1
        return a_score(t) * self._net(t, Y[:, :9])

    def bound(self, t, Y):
        import torch
        sd, q = self.sd, "pose_score_net."
        x = torch.as_tensor(Y[:, :9])
        R = x.shape[0]
        u = U32
        W = lambda k: sd[q + k + ".weight"]
        B_ = lambda k: sd[q + k + ".bias"]

        def layer(key, v, e, relu=True):
            """value and error bound of (relu of) W v + b, v carrying error bound e; n products summed in float32"""
            w, b = W(key), B_(key)
            n = w.shape[1]
            val = v @ w.T + b
            mag = v.abs() @ w.abs().T + b.abs()
            err = e @ w.abs().T + (4 * np.sqrt(n) + 1) * u * mag
            return (val.clamp(min=0) if relu else val), err, mag

        # time features (sinf / cosf of a float32 argument up to |2 pi W t| ~ 1e2: a few u of the argument)
        Wt = sd[q + "t_encoder.0.W"]
        arg = float(t) * Wt * 2 * np.pi
        four = torch.cat([torch.sin(arg), torch.cos(arg)])[None, :]
        e_four = (8 * u * (arg.abs() + 1))[None, :].repeat(1, 2)
        tf, e_tf, _ = layer("t_encoder.1", four, e_four)
        h1, e1, _ = layer("pose_encoder.0", x, u * x.abs())  # float32 network input
        h2, e2, _ = layer("pose_encoder.2", h1, e1)
        total = torch.cat([self.feat[:R], tf.expand(R, -1), h2], dim=1)
        e_tot = torch.cat([torch.zeros(R, 1024, dtype=torch.float64), e_tf.expand(R, -1), e2], dim=1)
        errs = []
        for h in ("rot_x", "rot_y", "trans"):
            p = f"fusion_tail_{h}"
            z, ez, _ = layer(p + ".0", total, e_tot)
            o, eo, mo = layer(p + ".2", z, ez, relu=False)
            errs.append(eo)
        err = torch.cat(errs, dim=1).numpy()
        f = self._net(t, Y[:, :9])
        # float32 sigma (powf of a float32 t: < 16 u) and the division
        return abs(a_score(t)) * (err + 20 * u * np.abs(f))


def exact_f32_problem():
    """An analytic field the float32 network evaluates EXACTLY: A diagonal with power-of-two entries, no offset, no time term.  Every
    layer sum then has one nonzero product (a power-of-two scaling), so the device's f_theta is A . float32(stage state) to the bit,
    and its stage derivative -g^2/2 . f / (sigma + 1e-7) carries only the rounding of one float32 division and of sigma: a bound of
    a few u, tight enough to see a Dormand-Prince coefficient off by 1e-6."""
    diag = -np.array([2.0 ** -2, 2.0 ** -3, 2.0 ** -3, 2.0 ** -4, 2.0 ** -2, 2.0 ** -5, 2.0 ** -3, 2.0 ** -4, 2.0 ** -2])
    return AnalyticNet(np.diag(diag), np.zeros((9, len(CHANS))), CHANS)


def robust_schedule(field, t0, Y0, t1, rtol=1e-5, atol=1e-5, seeds=3, scale=0.25):
    """Does the float64 schedule survive float32-size noise in every evaluation?  Replays the whole solve with each evaluation
    perturbed by scale x its float32 bound (uniform, fixed seed) and compares accept / reject sequence and evaluation count with the
    unperturbed run.  A problem whose schedule changes under such noise is path-sensitive: a float32 device cannot be held to scipy's
    schedule on it, only to the float64 replay of its own attempts."""
    R = Y0.shape[0]
    base = fun_flat(field, R)
    ref, _ = replay_run(base, t0, Y0.reshape(-1), t1, rtol, atol)
    for s in range(seeds):
        rng = np.random.default_rng(1000 + s)

        def noisy(t, y):
            b = field.bound(t, y.reshape(R, field.nc)).reshape(-1)
            return base(t, y) + scale * b * rng.uniform(-1, 1, y.size)

        got, _ = replay_run(noisy, t0, Y0.reshape(-1), t1, rtol, atol)
        if [a["acc"] for a in got] != [a["acc"] for a in ref]:
            return False
    return True
