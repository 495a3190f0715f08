"""Networks driven by piecewise-linear input time courses for the tests of MassActionODELogLike(inputs=...): a two-species linear drive,
and the networks of ode_networks, ode_wide_networks and ode_wave_networks with one or two input species that catalyse a production (and a
degradation).  All synthetic.  The references share no code with the solver under test:

  * piecewise_radau: ode_reference.radau called segment by segment between the knots (and the event times).  ode_reference.radau
    integrates autonomous mass action only, so the input g * interp(t) is carried through a segment as what it is there, a straight line:
    a reference species set to g * interp(tau) by hand at the segment's start and fed by a zero-order source whose rate constant is the
    segment's slope g * s_k (a plain number in the reference's own right-hand side; negative on a falling segment).  Radau integrates
    that line to its own tolerance (1e-12), so every other species sees g * interp(t);
  * drive2_closed_form: for A' = k_in g u(t) - k_d A the exact solution, segment by segment."""
import functools

import numpy as np

from pydream_amd.likelihoods import Input, MassActionODELogLike, Monomial

from . import ode_networks as NW
from . import ode_reference as R
from . import ode_wide_networks as W

# outputs at 0.5, 1.0, ..., 10 from t0 = 0 (Michaelis-Menten, enzyme13, drive2): the first table time before t0, a knot BETWEEN two outputs
# (0.75, 4.2), a knot exactly ON the output time 3.0, a falling segment that ends at 0 (at 7.0, on an output) followed by a flat one, the
# last table time after t[-1]
PULSE_T, PULSE_V = (-1.0, 0.75, 3.0, 4.2, 7.0, 12.0), (0.2, 0.2, 1.5, 1.5, 0.0, 0.0)
# outputs at 0, 0.5, ..., 5 from t0 = 0 (the chains; an output at t0): the same features, the knot on an output at 1.5, the fall ends at 3.7
CHAIN_PULSE_T, CHAIN_PULSE_V = (-0.5, 0.3, 1.5, 2.2, 3.7, 6.0), (0.1, 0.1, 1.0, 1.0, 0.0, 0.0)
# a second input for chain40: a ramp up and a plateau (2 working knots inside the span, one of them at the other input's 2.2)
RAMP_T, RAMP_V = (0.0, 2.2, 5.0), (0.0, 0.6, 0.6)
K_IN, GAIN = np.log10(0.8), np.log10(1.5)      # the nominal log10 production constant and gain, the two parameters every network here adds
DRIVE2_T = np.linspace(0.5, 10.0, 20)
DRIVE2_NOMINAL = np.array([K_IN, np.log10(0.6), GAIN])     # k_in, k_d, gain
MM_STARVED_MAX_STEPS = 40   # per SEGMENT: in the +-1 decade box some points fail in all three conditions, some in a few, some in none
                            # (chosen on the host build: test_ode_inputs_cpu.test_a_starved_step_limit_fails_a_mix_of_conditions)
MM_EVENTS = ((0.25, 1, 1.0, 1.0), (3.0, 1, 1.0, 1.5), (6.2, 1, 0.0, 0.0))      # ode_event_networks.MM_EVENTS: before, on and between outputs
# Michaelis-Menten's three conditions: tables of 2, 3 and 6 knots (so 1, 2 and 5 working knots), the last one also with the three events
MM_CONDITION_TABLES = (((-1.0, 12.0), (0.4, 0.4)), ((0.0, 3.0, 10.0), (0.0, 1.2, 0.3)), (PULSE_T, PULSE_V))
MM_CONDITION_EVENTS = ((), (), MM_EVENTS)


def network(name):
    """dict(S, rx, y0, t, obs, nominal, lanes, inputs, sd_rel) of a named network.  The input species come last; the production constant
    is parameter P and the gain parameter P + 1, P the parameter count of the network underneath; the observables are the network's own
    and, last, the input species themselves."""
    if name == "drive2":            # U, A:  U -> U + A (k_in),  A -> 0 (k_d),  gain 10**x[2]
        return dict(S=2, rx=[({0: 1}, {0: 1, 1: 1}, 0), ({1: 1}, {}, 1)], y0=np.zeros(2), t=DRIVE2_T, obs=np.eye(2)[::-1].copy(), nominal=DRIVE2_NOMINAL,
                    lanes=1, inputs=[Input(0, PULSE_T, PULSE_V, gain=2)], sd_rel=0.05)
    if name == "mm":                # the input produces substrate
        S, rx, y0, t, obs, nominal, lanes, sd_rel = 4, NW.MM_REACTIONS, NW.MM_Y0, NW.MM_T, [[0, 1, 0, 0], [0, 0, 0, 1]], NW.MM_NOMINAL, 1, 0.05
        target, pulse = 1, (PULSE_T, PULSE_V)
    elif name == "enzyme13":        # ... substrate A
        ENZ = W.ENZ
        S, rx, y0, t, obs, nominal, lanes, sd_rel = 13, ENZ.REACTIONS, ENZ.Y0, ENZ.TSPAN, ENZ.OBSERVABLES, ENZ.NOMINAL, 16, 0.03
        target, pulse = ENZ.A, (PULSE_T, PULSE_V)
    else:                           # chain17, chain40: the input produces species 0, and the last species is degraded (a resting state exists)
        S = int(name[5:])
        rx, y0, obs = W.chain_network(S)
        rx = list(rx) + [({S - 1: 1}, {}, 0.5)]
        t, nominal, lanes, sd_rel, target, pulse = W.CHAIN_T, W.CHAIN_NOMINAL, 32 if S <= 32 else 64, 0.03, 0, (CHAIN_PULSE_T, CHAIN_PULSE_V)
    P, U = len(nominal), S
    rx = list(rx) + [({U: 1}, {U: 1, target: 1}, P)]
    inputs = [Input(U, *pulse, gain=P + 1)]
    if name == "chain40":           # a second input, without a sampled gain, that catalyses the degradation of species S // 2
        rx.append(({U + 1: 1, S // 2: 1}, {U + 1: 1}, 0.7))
        inputs.append(Input(U + 1, RAMP_T, RAMP_V, gain=Monomial({P: 1}, 0.25)))
    n = len(inputs)
    obs = np.asarray(obs, dtype=float)
    obs = np.block([[obs, np.zeros((len(obs), n))], [np.zeros((n, S)), np.eye(n)]])
    return dict(S=S + n, rx=rx, y0=np.r_[np.asarray(y0, dtype=float), np.zeros(n)], t=np.asarray(t, dtype=float), obs=obs,
                nominal=np.r_[nominal, K_IN, GAIN], lanes=lanes, inputs=inputs, sd_rel=sd_rel)


def gains(inputs, x, log10=True):
    """the gains g_i at the point x as doubles (numpy's arithmetic: the reference's own)"""
    out = []
    for u in inputs:
        g = u.gain
        out.append(1.0 if g is None else float(g.value(x)) if isinstance(g, Monomial) else g if isinstance(g, float) else
                   10.0 ** x[g] if log10 else x[g])
    return out


def input_curve(u, g, t):
    """g * interp(t): what the input species is at the times t"""
    return g * np.interp(t, u.times, u.values)


def piecewise_radau(S, reactions, k, y0, t, inputs, g, events=(), t0=0.0, **kw):
    """The states at the output times t, [T, S] (the module's head): ode_reference.radau restarted at every knot and every event time.
    An output at an event's time is the state before the event."""
    t = np.asarray(t, dtype=float)
    y = np.array(y0, dtype=float)
    rx = list(reactions) + [({}, {u.species: 1}, 0.0) for u in inputs]

    def slope(u, tau):              # of the segment that follows tau
        j = int(np.clip(np.searchsorted(u.times, tau, side="right") - 1, 0, len(u.times) - 2))
        return (u.values[j + 1] - u.values[j]) / (u.times[j + 1] - u.times[j])

    def intervene(y, tau):
        for u, gi in zip(inputs, g):
            y[u.species] = gi * np.interp(tau, u.times, u.values)
        for time, s, factor, amount in events:
            if time == tau:
                y[s] = factor * y[s] + amount

    intervene(y, t0)
    out, done, now = np.empty((len(t), S)), np.zeros(len(t), dtype=bool), t0
    breaks = sorted({tau for u in inputs for tau in u.times if t0 < tau < t[-1]} | {e[0] for e in events if t0 < e[0] < t[-1]})
    for tau in breaks + [None]:
        end = t[-1] if tau is None else tau
        take = ~done & (t <= end)
        kk = np.r_[k, [gi * slope(u, now) for u, gi in zip(inputs, g)]]
        ys = R.radau(S, rx, kk, y, np.r_[t[take], end], t0=now, **kw)
        out[take], done = ys[:-1], done | take
        y, now = ys[-1].copy(), end
        if tau is not None:
            intervene(y, tau)
    assert done.all()
    return out


def radau_observed(args):
    """(S, reactions, y0, t, inputs, events, t0, observables, x) -> the observables [T, O] at the log10 constants x; for a process pool"""
    S, rx, y0, t, inputs, events, t0, obs, x = args
    y = piecewise_radau(S, rx, R.rate_constants(rx, x, "log10"), y0, t, inputs, gains(inputs, x), events, t0)
    return y @ np.asarray(obs, dtype=float).T


def drive2_closed_form(x, t, u, t0=0.0):
    """A(t) of A' = k_in g u(t) - k_d A, A(t0) = 0, exactly: on a segment u = a + b (t - tau),
    A = A_tau e^(-k_d dt) + k_in g (a E + b (dt - E) / k_d),  E = (1 - e^(-k_d dt)) / k_d."""
    k_in, k_d, g = (10.0 ** v for v in x[:3])
    knots = [t0] + [tau for tau in u.times if t0 < tau]
    out = np.empty(len(t))
    for j, tj in enumerate(t):
        A, now = 0.0, t0
        for nxt in knots[1:] + [np.inf]:
            end = min(nxt, tj)
            dt, a = end - now, float(np.interp(now, u.times, u.values))
            b = (float(np.interp(end, u.times, u.values)) - a) / dt if dt > 0 else 0.0
            E = -np.expm1(-k_d * dt) / k_d
            A, now = A * np.exp(-k_d * dt) + k_in * g * (a * E + b * (dt - E) / k_d), end
            if end == tj:
                break
        out[j] = A
    return out


@functools.lru_cache(maxsize=None)
def _data(name, tables, events, t0):
    """The observables [O, T] of a named network at its nominal constants under the tables (one (times, values) per input) and events"""
    n = network(name)
    inputs = [Input(u.species, tau, v, gain=u.gain) for u, (tau, v) in zip(n["inputs"], tables)]
    return radau_observed((n["S"], n["rx"], n["y0"], n["t"], inputs, events, t0, n["obs"], n["nominal"])).T.copy()


def _tables(inputs):
    return tuple((u.times, u.values) for u in inputs)


def single(name, inputs="own", events=None, t0=0.0, data=None, **kw):
    """The named network as a single experiment, its data piecewise Radau's at the nominal constants under the same inputs and events.
    inputs: a list of Input, or "own" for the network's; None: the keyword is not passed at all (then data must be given)."""
    n = network(name)
    inputs = n["inputs"] if isinstance(inputs, str) else inputs
    if data is None:
        data = _data(name, _tables(inputs), tuple(events or ()), float(t0))
    kw.setdefault("lanes_per_point", n["lanes"])
    if inputs is not None:
        kw["inputs"] = list(inputs)
    if events is not None:
        kw["events"] = list(events)
    return MassActionODELogLike(n["S"], n["rx"], n["y0"], n["t"], n["obs"], data, n["sd_rel"] * np.abs(data) + 0.01, t0=t0, **kw)


def conditions(name, tables, events, **kw):
    """(multi, one): `name` under one condition per entry of `tables` (the (times, values) of its first input) with events[c];
    one(c, **kw2) is the single-experiment object of condition c with the same data."""
    n = network(name)
    own, conds, each = n["inputs"], [], []
    for (tau, v), ev in zip(tables, events):
        inputs = [Input(own[0].species, tau, v, gain=own[0].gain)] + own[1:]
        data = _data(name, _tables(inputs), tuple(ev), 0.0)
        each.append(inputs)
        conds.append(dict(data=data, sd=n["sd_rel"] * np.abs(data) + 0.01, events=list(ev), inputs=inputs))
    shared = dict(lanes_per_point=n["lanes"])
    multi = MassActionODELogLike(n["S"], n["rx"], n["y0"], n["t"], n["obs"], None, None, conditions=conds, inputs=own, **dict(shared, **kw))

    def one(c, **kw2):
        return MassActionODELogLike(n["S"], n["rx"], n["y0"], n["t"], n["obs"], conds[c]["data"], conds[c]["sd"], events=conds[c]["events"],
                                    inputs=each[c], **dict(shared, **dict(kw, **kw2)))
    return multi, one


def mm_conditions(**kw):
    return conditions("mm", MM_CONDITION_TABLES, MM_CONDITION_EVENTS, **kw)


def enzyme13_conditions(**kw):
    """enzyme13 + input under the three tables of Michaelis-Menten's conditions, no events: the groups of a wave hold different knot times"""
    return conditions("enzyme13", MM_CONDITION_TABLES, ((), (), ()), **kw)


def emulation(name, slope=0.15, **kw):
    """What the code before inputs existed could build in the place of `name`: the same species and reactions, the input species plain
    species fed by a fixed zero-order source -- a single rising ramp.  For the register and scratch comparison and the rate tool."""
    n = network(name)
    rx = list(n["rx"]) + [({}, {u.species: 1}, float(slope)) for u in n["inputs"]]
    data = np.ones((len(n["obs"]), len(n["t"])))
    kw.setdefault("lanes_per_point", n["lanes"])
    return MassActionODELogLike(n["S"], rx, n["y0"], n["t"], n["obs"], data, data, ndim=len(n["nominal"]), **kw)
