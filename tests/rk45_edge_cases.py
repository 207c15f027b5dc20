"""The edge problems of the RK45 step controller (csrc/rk45.hip: rk45_decide_kernel, begin_attempt, rk45_record_kernel; samplers.py:
ODESampler._solve / run): analytic fields (rk45_reference.AnalyticNet) chosen so that scipy.integrate.RK45 on the float64 field takes a
named boundary branch of rk.py / common.py.  tests/test_rk45_edge_cases_cpu.py holds the float64 reference to every condition listed
here; tests/test_gpu_rk45_controller_edges.py holds the device to the reference.  A plain helper module (not collected by pytest).

Branches (the names used in Edge.branches and counted by branch_counts):
  h0_tiny     select_initial_step: d0 < 1e-5 or d1 < 1e-5 -> h0 = 1e-6
  h1_tiny     select_initial_step: d1 <= 1e-15 and d2 <= 1e-15 -> h1 = max(1e-6, 1e-3 h0)
  interval    h0 / h_abs clamped to |t_bound - t0|: the first attempt spans the whole interval and t_new = t_bound exactly
  min_step    h_abs < 10 ulp(t) without a preceding rejection: clamped up to min_step (then clipped to t_bound)
  err_zero    err_norm == 0 -> factor MAX_FACTOR
  cap         accepted with 0 < err_norm and 0.9 err^-0.2 > MAX_FACTOR -> factor MAX_FACTOR
  clamp       accepted right after a rejection with 0.9 err^-0.2 > 1 -> factor min(1, .) = 1
  log_cap     more than 512 attempts: the device's per-attempt log stops filling, the solve goes on
  traj_cap    more accepted states than ODESampler.TRAJ_CAP
  dense_one   dense output with one t_eval point (t_eval = [T0])
No AnalyticNet field reaches the MIN_FACTOR floor (err_norm > (0.9 / 0.2)^5 ~ 1845) with finite data - select_initial_step keeps the
first attempt's error far below that on smooth fields, and a rejected attempt shrinks the step; search_min_factor_floor() is the search
the CPU test runs.  The floor is reached on the device by the non-finite-state case only (fmax(MIN_FACTOR, NaN) = MIN_FACTOR)."""
import math
from dataclasses import dataclass

import numpy as np

import rk45_reference as rr

LOG_CAP = 512  # Rk45State::log_*[512]
SHAPES = [(2, 3), (3, 43)]  # clouds x candidates: 6 rows on the 16-row tile plan, 129 rows on the 128-row chain plan (two workgroups)
PLAN_OF_SHAPE = {(2, 3): 16, (3, 43): 128}


@dataclass
class Edge:
    name: str
    problem: str                 # key of nets()
    model: str                   # driver model ('score' | 'likelihood')
    T0: float
    t_bound: float
    branches: tuple              # branch names the float64 scipy solve must take at least once
    strict: bool                 # error norms stay away from 1: the device must take scipy's accept / reject sequence and nfev exactly
    rtol: float = 1e-5
    atol: float = 1e-5
    zero_state: bool = False     # initial state all zero instead of the prior draw
    exact: bool = False          # every logged quantity is exact (zero field): log_t / log_h bit-equal to scipy's, end state == y0
    shapes: tuple = tuple(SHAPES)
    num_steps: int = 0           # dense output points (dense_one)
    max_attempts: int = 4096     # attempt budget the device solve runs under (ODESampler's default)


def nets():
    """name -> AnalyticNet, built like rk45_reference.problems() (same seeds, same A / Cw / d)"""
    base = rr.problems()
    contract, time, lik = base["contract"][0], base["time"][0], base["likelihood"][0]
    nch = len(rr.CHANS)
    z9, zc = np.zeros((9, 9)), np.zeros((9, nch))
    return {
        "contract": contract,
        "likelihood": lik,
        "zero": rr.AnalyticNet(z9, zc, rr.CHANS),                       # f_theta = 0
        "offset_only": rr.AnalyticNet(z9, contract.Cw, rr.CHANS),       # f_theta = c_cloud: the right-hand side depends on t alone
        # the same with offsets of 1e-6 the size: the float32 noise of an attempt's error norm (proportional to |f| / atol) then stays
        # orders of magnitude below the error norm at which the MAX_FACTOR cap lets go, (0.9 / 10)^5 ~ 5.9e-6
        "offset_small": rr.AnalyticNet(z9, 1e-6 * contract.Cw, rr.CHANS),
        "time30": rr.AnalyticNet(time.A, time.Cw, rr.CHANS, d=time.d, omega=30.0),
        "time130": rr.AnalyticNet(time.A, time.Cw, rr.CHANS, d=time.d, omega=130.0),
        "time400": rr.AnalyticNet(time.A, time.Cw, rr.CHANS, d=time.d, omega=400.0),
    }


EPS = rr.EPS
# eps + 5 ulp(eps): the whole interval is shorter than min_step = 10 ulp(T0)
T0_MIN_STEP = float(EPS + 5 * np.spacing(EPS))

EDGES = [
    Edge("zero_field", "zero", "score", 1.0, EPS, ("h0_tiny", "h1_tiny", "err_zero"), True, exact=True),
    Edge("zero_field_likelihood", "zero", "likelihood", EPS, 1.0, ("h0_tiny", "h1_tiny", "err_zero"), True, exact=True),
    # (with the offsets of 'contract' the capped attempts' error norms - 4.7e-6 at h = 1e-2 - lie inside the float32 noise of the cap's
    # threshold 5.9e-6: the schedule changes under float32-size noise, so that solve is held to the float64 replay only)
    Edge("zero_state", "offset_only", "score", 0.55, EPS, ("h0_tiny", "cap"), False, zero_state=True),
    Edge("zero_state_small_offset", "offset_small", "score", 0.55, EPS, ("h0_tiny", "cap"), True, zero_state=True),
    Edge("interval_2e-5", "contract", "score", 2e-5, EPS, ("interval",), True),
    Edge("interval_1.00001e-5", "contract", "score", 1.00001e-5, EPS, ("interval",), True),
    Edge("interval_1e-4", "contract", "score", 1e-4, EPS, ("interval",), True),
    Edge("interval_likelihood", "likelihood", "likelihood", 1.0 - 1e-6, 1.0, ("interval",), True),
    Edge("min_step", "contract", "score", T0_MIN_STEP, EPS, ("interval", "min_step"), True),
    Edge("clamp_after_reject", "time30", "score", 0.15, EPS, ("clamp",), False),
    Edge("traj_overflow", "time130", "score", 1.0, EPS, ("traj_cap",), False, shapes=((2, 3),)),
    # rtol = atol = 1e-9 is below what a float32 network resolves: the float32 noise of the stage derivatives alone puts the error norm
    # over 1 until the steps are several times shorter than the float64 schedule's (the restated controller with 1 % - 5 % of the
    # float32 bound as noise in every evaluation takes 1 600 - 6 600 attempts for the 568 of float64), so the device runs this one under
    # a larger budget; log_overflow_f32 is the same branch at a tolerance the device follows attempt for attempt
    Edge("log_overflow", "time30", "score", 1.0, EPS, ("log_cap",), False, rtol=1e-9, atol=1e-9, shapes=((2, 3),), max_attempts=32768),
    Edge("log_overflow_f32", "time400", "score", 1.0, EPS, ("log_cap",), False, shapes=((2, 3),)),
    Edge("dense_one_point", "contract", "score", 0.55, EPS, ("dense_one",), False, num_steps=1),
]
BY_NAME = {e.name: e for e in EDGES}
# (entry, clouds, candidates) of every solve the tests run
CASES = [(e.name, B, K) for e in EDGES for (B, K) in e.shapes]


class EdgeField(rr.Field):
    """rr.Field whose float32 bound also carries the rounding of the time feature's ARGUMENT: the device evaluates tau(t) = sin(x) + 2 at
    x = float32(t) . omega . 2 . pi, three float32 roundings of a number up to 2 pi omega.  At omega = 3 (rr.problems()) that is inside
    the 32 u of the summed magnitudes rr.Field.bound allows; at omega = 30 - 130 and t near 1 it is not: |x| u = 817 u at omega = 130 (an
    accepted state of that solve measured 1.53 x rr.Field's bound on an MI355X).  The term is the one rr.NetField.bound uses for the
    same arithmetic, 8 u (|x| + 1) per time feature, through |d| and a(t)."""

    def bound(self, t, Y):
        b = super().bound(t, Y)
        net = self.net
        if net.d is not None:
            arg = abs(2 * np.pi * net.omega * t)
            a = abs(rr.a_energy(t) if self.model == "energy" else rr.a_score(t))
            b[:, :9] += a * np.abs(net.d) * 8 * rr.U32 * (arg + 1)
        return b


def setup(edge, B, K, seed=0):
    """-> dict(net, model, pf, x [R,9] f32, probe, c_rows, field (float64 right-hand side), Y0 [R,nc] f64)"""
    if isinstance(edge, str):
        edge = BY_NAME[edge]
    net = nets()[edge.problem]
    lik = edge.model == "likelihood"
    pf, x, probe = rr.inputs(B, K, edge.T0, seed=seed, likelihood=lik)
    if edge.zero_state:
        x = np.zeros_like(x)
    c_rows = np.repeat(net.offsets(pf), K, 0)
    fld = EdgeField(net, edge.model, c_rows, probe if lik else None)
    Y0 = np.concatenate([x, np.zeros((B * K, 1))], 1).astype(np.float64) if lik else x.astype(np.float64)
    return dict(edge=edge, net=net, model=edge.model, pf=pf, x=x, probe=probe, c_rows=c_rows, field=fld, Y0=Y0)


def scipy_reference(p):
    e, Y0 = p["edge"], p["Y0"]
    return rr.scipy_run(rr.fun_flat(p["field"], Y0.shape[0]), e.T0, Y0.reshape(-1), e.t_bound, e.rtol, e.atol)


def raw_factor(err):
    return rr.SAFETY * err ** rr.ERR_EXP


def branch_counts(sc, T0, t_bound):
    """How often a scipy_run log (or a device log with the same keys: err, acc, h) takes each branch that shows from the outside."""
    err, acc, h = np.asarray(sc["err"], dtype=np.float64), np.asarray(sc["acc"], dtype=bool), np.asarray(sc["h"], dtype=np.float64)
    n = len(acc)
    with np.errstate(divide="ignore"):
        raw = np.where(err > 0, rr.SAFETY * np.where(err > 0, err, 1.0) ** rr.ERR_EXP, np.inf)
    after_reject = np.concatenate([[False], ~acc[:-1]]) if n else np.zeros(0, dtype=bool)
    return dict(
        attempts=n, accepted=int(acc.sum()),
        err_zero=int(np.sum(err == 0)),
        cap=int(np.sum(acc & (err > 0) & (raw > rr.MAX_FACTOR))),
        clamp=int(np.sum(acc & after_reject & (raw > 1))),
        floor=int(np.sum(~acc & (raw < rr.MIN_FACTOR))),
        interval=int(n > 0 and abs(h[0]) == abs(t_bound - T0)),
        log_cap=int(n > LOG_CAP),
    )


def initial_step_of(p):
    """rr.initial_step on the float64 field from the problem's y0 -> (h0, h_abs, d0, d1, d2)"""
    e, Y0 = p["edge"], p["Y0"]
    fun = rr.fun_flat(p["field"], Y0.shape[0])
    y = Y0.reshape(-1)
    return rr.initial_step(e.T0, y, fun(e.T0, y), fun, e.t_bound, e.rtol, e.atol)


def min_ln_err(sc):
    err = np.asarray(sc["err"], dtype=np.float64)
    err = err[err > 0]
    return float(np.min(np.abs(np.log(err)))) if err.size else math.inf


def err_margins(p, sc):
    """per attempt of the float64 solve: (|err - 1|, rr.err_noise band) - the margin test_strict_problems_keep_err_norm_away_from_one uses"""
    e, Y0 = p["edge"], p["Y0"]
    fun = rr.fun_flat(p["field"], Y0.shape[0])
    out, k = [], 0
    for t, h, acc in zip(sc["t"], sc["h"], sc["acc"]):
        y = sc["states"][k]
        _, _, _, err, stage_y = rr.dp_attempt(fun, t, y, fun(t, y), h, e.rtol, e.atol)
        out.append((abs(err - 1.0), rr.err_noise(p["field"], t, y, h, stage_y, e.rtol, e.atol)))
        k += int(acc)
    return out


def halving_attempts(T0, t_bound):
    """Attempts of a solve whose every error norm is NaN: the first attempt spans the whole interval (fmin(NaN, interval) = interval in the
    initial step), each attempt is rejected with factor fmax(MIN_FACTOR, NaN) = MIN_FACTOR, and the solve fails at the first attempt
    start with h_abs < min_step = 10 ulp(T0) - after ceil(ln(interval / min_step) / ln(1 / MIN_FACTOR)) attempts; + 1 for an exact
    power (h_abs == min_step is not 'less than')."""
    direction = np.sign(t_bound - T0)
    min_step = 10 * abs(np.nextafter(T0, direction * np.inf) - T0)
    return int(math.ceil(math.log(abs(t_bound - T0) / min_step) / math.log(1.0 / rr.MIN_FACTOR))) + 1


def search_min_factor_floor():
    """Looks for a finite AnalyticNet problem whose float64 solve has a rejected attempt at the MIN_FACTOR floor: stiff and strongly
    forced variants of the fields above at loose and tight tolerances.  -> list of (description, rejected-at-floor count)."""
    base = rr.problems()
    time = base["time"][0]
    found = []
    B, K = 2, 3
    for omega in (30.0, 100.0, 1000.0):
        for scale in (1.0, 50.0):
            for tol in (1e-5, 1e-2):
                for T0 in (1.0, 0.15):
                    net = rr.AnalyticNet(time.A * scale, time.Cw, rr.CHANS, d=time.d * scale, omega=omega)
                    pf, x, _ = rr.inputs(B, K, T0)
                    fld = rr.Field(net, "score", np.repeat(net.offsets(pf), K, 0))
                    try:
                        sc = rr.scipy_run(rr.fun_flat(fld, B * K), T0, x.astype(np.float64).reshape(-1), EPS, tol, tol)
                    except RuntimeError:
                        continue
                    n = branch_counts(sc, T0, EPS)["floor"]
                    if n:
                        found.append((f"omega={omega} scale={scale} tol={tol} T0={T0}", n))
    return found
