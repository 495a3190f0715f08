"""Networks for the tests of a STEADY OUTPUT, MassActionODELogLike(t=[..., inf], settle=...): the networks of ode_networks,
ode_wide_networks and ode_wave_networks with one more row measured at the steady state the experiment ends in, a modification cycle and
a receptor with turnover whose steady states are known in closed form, the Brusselator of ode_equilibrate_networks, and
ode_combined_networks' seeded cases with the steady row on top of every other feature.  All synthetic: the data are the host build's own
tight simulation at the nominal constants -- they only define a likelihood; what the tests compare against is numpy's restatement of the
steady-state test, an mpmath Newton iteration on the reference's right-hand side, scipy's Radau, closed forms and the host build's
bits.  Nothing here is collected."""
import functools

import numpy as np

from pydream_amd.likelihoods import Input, MassActionODELogLike

from . import ode_combined_networks as CB
from . import ode_equilibrate_networks as EQ
from . import ode_networks as NW
from . import ode_reference as R

INF = np.inf
WAVE = "chain33"        # the 64-lane network of the GPU cases
# Budgets of the phase's attempted steps at which, in the +-1 decade box around the nominal constants, at least a quarter of
# starved_points() fail and at least a quarter settle (chosen on the host build, from the attempts the points need at the default
# budget: test_ode_settle_cpu.test_a_starved_phase_fails_a_quarter_and_settles_a_quarter asserts both shares)
STARVED_SETTLE_STEPS = {"mm": 60, WAVE: 140}
STARVED_POINTS = 259


def network(name, identity=False):
    """ode_equilibrate_networks.network(name); identity: with the observables np.eye(S) (S <= the shape's observable limit)"""
    S, rx, y0, t, obs, nominal, sd_rel, lanes = EQ.network(name)
    return S, rx, y0, np.asarray(t, dtype=float), (np.eye(S) if identity else np.asarray(obs, dtype=float)), nominal, sd_rel, lanes


def with_steady_row(t):
    return np.r_[np.asarray(t, dtype=float), INF]


def _freeze(v):
    if isinstance(v, dict):
        return tuple(sorted((k, _freeze(x)) for k, x in v.items()))
    if isinstance(v, (list, tuple, np.ndarray)):
        return tuple(_freeze(x) for x in v)
    return v


@functools.lru_cache(maxsize=None)
def _data(name, obs, y0, events, horizon, steady_only):
    """The observables [O, T] of the named network, steady row included, at the nominal constants: the host build at tight tolerances
    (cached: the tests share them)."""
    S, rx, _, t, _, nominal, _, lanes = network(name)
    t = np.array([INF]) if steady_only else with_steady_row(t)
    obs = np.array(obs)
    tight = MassActionODELogLike(S, rx, np.array(y0), t, obs, np.full((len(obs), len(t)), np.nan), 1.0, lanes_per_point=lanes, events=list(events),
                                 settle=dict(horizon=horizon, max_steps=20000), rtol=1e-10, atol=1e-12, max_steps=20000)
    sim = tight.simulate(nominal)[0]
    assert np.all(np.isfinite(sim)), name
    return sim.T.copy()


def experiment(name, observables=None, y0=None, events=(), settle=None, steady_only=False):
    """dict(y0, data, sd, events) of one experiment of the named network whose last row is the steady one; settle: the horizon the data's
    own phase runs with (default: the experiment's length); steady_only: t = [inf]"""
    S, rx, own_y0, t, obs, _, sd_rel, _ = network(name)
    obs = obs if observables is None else np.asarray(observables, dtype=float)
    y0 = np.asarray(own_y0 if y0 is None else y0, dtype=float)
    horizon = float(settle.get("horizon", t[-1])) if isinstance(settle, dict) else float(t[-1])
    data = _data(name, _freeze(obs), tuple(y0), _freeze(list(events)), horizon, bool(steady_only))
    return dict(y0=y0, data=data, sd=sd_rel * np.abs(data) + 0.01, events=list(events))


def single(name, observables=None, y0=None, events=(), settle=None, steady_only=False, **kw):
    """The named network as one experiment with the steady row; settle: what the constructor gets."""
    S, rx, _, t, obs, _, _, lanes = network(name)
    obs = obs if observables is None else np.asarray(observables, dtype=float)
    e = experiment(name, obs, y0, events, settle, steady_only)
    return MassActionODELogLike(S, rx, e["y0"], [INF] if steady_only else with_steady_row(t), obs, e["data"], e["sd"], lanes_per_point=lanes,
                                events=e["events"], settle=settle, **kw)


def finite_twin(like, observables=None, **kw):
    """The object of `like` with the steady row cut off: t = [.., t_last], no phase -- what the parent commit could express."""
    obs = like.observables if observables is None else np.asarray(observables, dtype=float)
    T = len(like.t) - 1
    data = like.data[:, :T] if observables is None else np.full((len(obs), T), np.nan)
    sd = like.sd[:, :T] if observables is None else np.ones((len(obs), T))
    return MassActionODELogLike(like.n_species, like.reactions, like.y0, like.t[:-1], obs, data, sd, rate_scale=like.rate_scale, t0=like.t0,
                                rtol=like.rtol, atol=like.atol, max_steps=like.max_steps, lanes_per_point=like.lanes_per_point, events=like.events,
                                inputs=like.inputs, **kw)


def equilibrating_from(like, y, observables=None):
    """The second object of the hand-over identity (csrc/dz_ode.h, STEADY OUTPUT, point 2): the same network started from y0 = y with
    `equilibrate` set to the five numbers of like.settle and t = [t0].  y goes straight into the object's block, as in
    ode_equilibrate_networks.plain_from: a state may carry an amount that is negative within the solver's tolerance."""
    obs = like.observables if observables is None else np.asarray(observables, dtype=float)
    twin = MassActionODELogLike(like.n_species, like.reactions, np.zeros(like.n_species), [like.t0], obs, np.full((len(obs), 1), np.nan), 1.0,
                                rate_scale=like.rate_scale, t0=like.t0, rtol=like.rtol, atol=like.atol, max_steps=like.max_steps,
                                lanes_per_point=like.lanes_per_point, equilibrate=dict(like.settle))
    twin.y0 = np.array(y, dtype=float)
    return twin


def mm_conditions(**kw):
    """(multi, one): Michaelis-Menten with identity observables under three conditions that all end in a steady row -- the plain
    experiment, a double dose of substrate, and a wash-out of the product with a bolus of substrate AT t_last (measure, intervene, let it
    settle); one(c): the single-experiment object of condition c."""
    S, rx, y0, t, obs, _, _, lanes = network("mm", identity=True)
    y0 = np.asarray(y0, dtype=float)
    t_last = float(t[-1])
    specs = [dict(), dict(y0=y0 * [1.0, 2.0, 1.0, 1.0]), dict(events=[(t_last, 3, 0.0, 0.0), (t_last, 1, 1.0, 1.0)])]
    exps = [experiment("mm", obs, **spec) for spec in specs]
    multi = MassActionODELogLike(S, rx, None, with_steady_row(t), obs, None, None, lanes_per_point=lanes, conditions=exps, **kw)

    def one(c, **kw2):
        e = exps[c]
        return MassActionODELogLike(S, rx, e["y0"], with_steady_row(t), obs, e["data"], e["sd"], lanes_per_point=lanes, events=e["events"],
                                    **dict(kw, **kw2))
    return multi, one


def starved(name, **kw):
    """The named network with the phase's budget at STARVED_SETTLE_STEPS[name]"""
    return single(name, settle=dict(max_steps=STARVED_SETTLE_STEPS[name]), **kw)


def starved_points(name):
    return NW.box_points(network(name)[5], STARVED_POINTS, 61, width=1.0)


# ---------------------------------------------------------------- closed forms
# The modification cycle X + E -> Xp + E (k1), Xp -> X (k2); species X, Xp, E: Xp* = Xtot k1 E / (k1 E + k2)
CYCLE_REACTIONS = [({0: 1, 2: 1}, {1: 1, 2: 1}, 0), ({1: 1}, {0: 1}, 1)]
CYCLE_NOMINAL = np.log10([2.0, 0.7])
# A receptor with turnover: 0 -> R (ksyn), R -> 0 (kdeg), R + L -> C (kon), C -> R + L (koff), C -> L (kint: the complex is
# internalised and the ligand recycled); species R, L, C.  At rest R* = ksyn / (kdeg + kint Q L*), C* = Q R* L*, Q = kon / (koff + kint),
# with L* + C* = Ltot
RECEPTOR_REACTIONS = [({}, {0: 1}, 0), ({0: 1}, {}, 1), ({0: 1, 1: 1}, {2: 1}, 2), ({2: 1}, {0: 1, 1: 1}, 3), ({2: 1}, {1: 1}, 4)]
RECEPTOR_NOMINAL = np.log10([1.0, 0.5, 2.0, 0.4, 0.8])


def cycle(E=1.5, horizon=4.0, **kw):
    """the modification cycle at kinase dose E: a pure steady-state measurement of all three species, t = [inf]"""
    return MassActionODELogLike(3, CYCLE_REACTIONS, [1.2, 0.0, E], [INF], np.eye(3), np.full((3, 1), 0.5), 0.1, settle=dict(horizon=horizon), **kw)


def cycle_closed_form(x, E=1.5, total=1.2):
    k1, k2 = 10.0 ** np.asarray(x, dtype=float)[..., 0], 10.0 ** np.asarray(x, dtype=float)[..., 1]
    xp = total * k1 * E / (k1 * E + k2)
    return np.stack([total - xp, xp, np.full_like(xp, E)], axis=-1)


def receptor(horizon=6.0, **kw):
    t = with_steady_row(np.linspace(1.0, 6.0, 6))
    return MassActionODELogLike(3, RECEPTOR_REACTIONS, [0.0, 1.0, 0.0], t, np.eye(3), np.full((3, len(t)), 0.5), 0.1, settle=dict(horizon=horizon), **kw)


# ---------------------------------------------------------------- the reference's own steady state
def drift(S, reactions, k, y, horizon, rtol, atol, ulps=0.0):
    """mean((f(y) horizon / (atol + rtol |y|))**2) in numpy: the steady-state test, written independently of the generated code
    (test_ode_equilibrate_cpu's _drift).  ulps: every |f_s| taken smaller by that many ulp of sum_j |N_sj| v_j, the magnitude of the
    terms that cancel in it."""
    N, nu = R.stoichiometry(S, reactions)
    v = k * np.prod(np.asarray(y, dtype=float)[None, :] ** nu, axis=1)
    f = np.maximum(np.abs(N @ v) - ulps * np.finfo(float).eps * (np.abs(N) @ np.abs(v)), 0.0)
    return float(np.mean((f * horizon / (atol + rtol * np.abs(y))) ** 2))


def newton_steady_state(S, reactions, k, y, dps=40, iterations=12):
    """(y*, ||(J|_V)^-1||_2): the steady state of the reference's right-hand side in the stoichiometric compatibility class of y -- y*
    = y + V z, V an orthonormal basis of range(N), by Newton's iteration on V^T f(y + V z) = 0 in dps-digit mpmath from z = 0 --, and
    the 2-norm of the inverse of the restricted Jacobian V^T J(y*) V in float64.  Nothing of the code under test is used but the
    starting point."""
    import mpmath
    mp = mpmath.mp
    N, _ = R.stoichiometry(S, reactions)
    U, sv, _ = np.linalg.svd(N.astype(float))
    V = U[:, :int(np.sum(sv > 1e-10 * sv[0]))]
    with mp.workdps(dps):
        Vm, km = mp.matrix(V.tolist()), [mp.mpf(float(v)) for v in k]
        ys = mp.matrix([mp.mpf(float(v)) for v in y])
        for _ in range(iterations):
            f, J = R._rhs_and_jacobian(S, reactions, km, list(ys), mp.mpf(0))
            g = Vm.T * mp.matrix(f)
            dz = mp.lu_solve(Vm.T * mp.matrix(J) * Vm, -g)
            ys = ys + Vm * dz
            if mp.norm(dz) < mp.mpf(10) ** (-dps + 8):
                break
        f, J = R._rhs_and_jacobian(S, reactions, km, list(ys), mp.mpf(0))
        assert mp.norm(mp.matrix(f)) < mp.mpf(10) ** (-dps // 2), "Newton's iteration did not converge"
        Jv = V.T @ np.array([[float(v) for v in row] for row in J]) @ V
        return np.array([float(v) for v in ys]), float(np.linalg.norm(np.linalg.inv(Jv), 2))


def first_t_big(S, reactions, ks, y0, horizon, rtol, atol, t0=0.0, start=1.0):
    """The first power of ten >= start at which Radau's state from (t0, y0) passes numpy's drift test at every one of the rate-constant
    rows ks; (t_big, the states there [n, S])."""
    t_big = start
    for _ in range(12):
        ys = np.array([R.radau(S, reactions, k, y0, [t0 + t_big], t0=t0)[0] for k in ks])
        if all(drift(S, reactions, k, y, horizon, rtol, atol) <= 1.0 for k, y in zip(ks, ys)):
            return t_big, ys
        t_big *= 10.0
    raise AssertionError("Radau did not come to rest")


def radau_at(S, reactions, k, y0, times, t0=0.0, rtol=1e-12, atol=1e-14):
    """ode_reference.radau -- scipy's Radau IIA at the same tolerances on the same right-hand side N v(y) -- with the Jacobian in
    numpy instead of ode_reference's plain loops, for runs over a thousand points of networks of 17 and 33 species: per (reaction,
    reactant) pair dv_r / dy_q = k_r c y_q^(c-1) prod_{s != q} y_s^nu_rs, J = sum over the pairs of N[:, r] dv at column q.  The
    states at `times` (ascending, > t0), [len(times), S]."""
    from scipy.integrate import solve_ivp
    N, nu = R.stoichiometry(S, reactions)
    k, N = np.asarray(k, dtype=float), N.astype(float)
    r_idx, q_idx = np.nonzero(nu)
    c = nu[r_idx, q_idx].astype(float)
    rest = nu[r_idx].astype(float)
    rest[np.arange(len(r_idx)), q_idx] = 0.0
    scatter = np.zeros((len(r_idx), S))
    scatter[np.arange(len(r_idx)), q_idx] = 1.0
    Nr = N[:, r_idx]

    def f(_, y):
        return N @ (k * np.prod(y[None, :] ** nu, axis=1))

    def jac(_, y):
        dv = k[r_idx] * c * y[q_idx] ** (c - 1.0) * np.prod(y[None, :] ** rest, axis=1)
        return (Nr * dv) @ scatter
    times = np.asarray(times, dtype=float)
    sol = solve_ivp(f, (t0, times[-1]), np.asarray(y0, dtype=float), method="Radau", t_eval=times, rtol=rtol, atol=atol, jac=jac)
    assert sol.success, sol.message
    return sol.y.T


# ---------------------------------------------------------------- everything together
COMBINED_SETTLE = dict(horizon=3.0, max_steps=4000)


class SteadyCase(CB.Case):
    """ode_combined_networks.Case with the steady row behind its twelve output times: conditions, a Monomial y0, events, equilibrate,
    Hill rate laws, sampled noise, inputs -- held at their value at t_last = 6.0 during the phase --, and on top a condition's "params"
    (steady_like) and the steady output."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.t = with_steady_row(CB.T_OUT)

    def steady_like(self, **kw):
        """the case's three conditions; condition 2 reads the scale Monomial's coordinate at the fixed value of the nominal point (a
        condition's "params") and carries a settle mapping of its own"""
        conds = [dict(data=d, sd=sd) for d, sd in self.data()]
        args = dict(rate_scale=self.rate_scale, t0=self.t0, lanes_per_point=self.lanes, ndim=CB.NDIM, scale=self.scale, noise=self.noise,
                    constraints=self.constraints, events=self.own_events, equilibrate=True, settle=COMBINED_SETTLE)
        args.update(kw)
        if self.U:
            args.setdefault("inputs", self.inputs[0])
        raw = [dict(data=conds[0]["data"], sd=conds[0]["sd"], events=[]),
               dict(data=conds[1]["data"], sd=conds[1]["sd"], y0=self.y0[1], equilibrate=False),
               dict(data=conds[2]["data"], sd=conds[2]["sd"], events=self.events[2], equilibrate=CB.EQUILIBRATE[2], params=self.view(),
                    settle=dict(COMBINED_SETTLE, max_steps=3000))]
        if self.U:
            raw[1]["inputs"], raw[2]["inputs"] = self.inputs[1], self.inputs[2]
        return MassActionODELogLike(self.S, self.reactions, self.y0[0], self.t, self.observables, None, None, conditions=raw, **args)

    def view(self):
        return {CB.P_SCALE: float(self.nominal[CB.P_SCALE])}

    def steady_single(self, c, **kw):
        """condition c of steady_like alone, made without "params": to be evaluated at the condition's viewed row"""
        kw.setdefault("settle", dict(COMBINED_SETTLE, max_steps=3000) if c == 2 else COMBINED_SETTLE)
        return self.single(c, **kw)

    def viewed(self, X, c):
        X = np.array(X, dtype=float)
        if c == 2:
            X[:, CB.P_SCALE] = self.nominal[CB.P_SCALE]
        return X


_steady_cases = {}


def steady_case(lanes):
    """the small full case of ode_combined_networks for the build, with the steady row"""
    if lanes not in _steady_cases:
        _steady_cases[lanes] = SteadyCase(*CB.CASES[next(i for i in CB.FULL if CB.CASES[i][0] == lanes)])
    return _steady_cases[lanes]


def input_held(ramp_after):
    """Michaelis-Menten whose enzyme production is driven by an input on a fifth species -- 0 -> E catalysed by U at rate 0.3, E -> 0 at
    0.4 --, with the steady row.  The input's table rises to (4.0, 1.0), has a knot ON t_last = 6.0 with the value 0.8, and after
    t_last either keeps falling to (9.0, 0.2) (ramp_after) or stays constant at 0.8: held with drive 0, both give the same bits."""
    rx = list(NW.MM_REACTIONS) + [({4: 1}, {4: 1, 0: 1}, 0.3), ({0: 1}, {}, 0.4)]
    table = ((0.0, 4.0, 6.0, 9.0), (0.1, 1.0, 0.8, 0.2 if ramp_after else 0.8))
    t = with_steady_row(np.linspace(1.0, 6.0, 6))
    return MassActionODELogLike(5, rx, list(NW.MM_Y0) + [0.0], t, np.eye(5), np.full((5, len(t)), 0.5), 0.1,
                                inputs=[Input(4, *table)], settle=dict(horizon=5.0, max_steps=4000))
