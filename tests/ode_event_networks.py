"""Networks with dosing and wash-out events for the tests of MassActionODELogLike(events=...): the networks of ode_networks,
ode_wide_networks and ode_condition_networks with interventions during the run.  All synthetic: the data come from scipy's Radau
RESTARTED at every event (ode_reference.radau called segment by segment, the state changed by hand in between), which shares no code with
the solver under test."""
import functools

import numpy as np

from pydream_amd.likelihoods import MassActionODELogLike

from . import ode_condition_networks as CN
from . import ode_networks as NW
from . import ode_reference as R
from . import ode_wide_networks as W

# Michaelis-Menten (outputs at 0.5, 1.0, ..., 10): a bolus of substrate BEFORE the first output, a second one exactly ON the output time
# 3.0, and a wash-out of the free substrate strictly BETWEEN the outputs 6.0 and 6.5
MM_EVENTS = ((0.25, 1, 1.0, 1.0), (3.0, 1, 1.0, 1.5), (6.2, 1, 0.0, 0.0))
# the 8-species chain (outputs at 0, 0.5, ..., 5): species 0 washed out between two outputs, species 7 on an output time
CHAIN8_EVENTS = ((1.25, 0, 0.0, 0.0), (2.0, 7, 0.0, 0.0))
# enzyme13 (outputs at 0.5, ..., 10): more substrate A before the first output, the inhibitor washed out on an output, B halved between two
ENZ_EVENTS = ((0.3, W.ENZ.A, 1.0, 2.0), (4.0, W.ENZ.I, 0.0, 0.0), (7.25, W.ENZ.B, 0.5, 0.0))
# chain17 (outputs at 0, 0.5, ..., 5): a wash-out between two outputs and a set-to-value on one
CHAIN17_EVENTS = ((0.75, 0, 0.0, 0.0), (2.5, 8, 0.0, 0.4))
# MM under the three doses of ode_condition_networks with 0, 1 and 3 events
MM_CONDITION_EVENTS = ((), ((2.2, 1, 0.0, 0.0),), MM_EVENTS)
# ... and enzyme13 under its three scales of A
ENZ_CONDITION_EVENTS = ((), ((4.0, W.ENZ.I, 0.0, 0.0),), ENZ_EVENTS)
# A step cap per SEGMENT at which, in the +-1 decade box around MM's nominal constants, some points fail in a segment after an event and
# others do not (chosen on the host build: test_ode_events_cpu.test_a_small_step_limit_fails_some_points_in_a_segment_after_an_event)
MM_STARVED_MAX_STEPS = 60


def piecewise_radau(S, reactions, k, y0, t, events, t0=0.0, **kw):
    """The states at the output times t, [T, S], by scipy's Radau restarted at every event time: integrate to the event, change the state
    by hand (factor * y + amount, events at one time in the order given), go on from there.  An output at an event's time is the state
    BEFORE the event; events at t0 change y0 (an output at t0 shows them)."""
    t = np.asarray(t, dtype=float)
    y = np.array(y0, dtype=float)
    events = sorted(events, key=lambda e: e[0])

    def intervene(y, tau):
        for time, s, factor, amount in events:
            if time == tau:
                y[s] = factor * y[s] + amount

    intervene(y, t0)
    out, done, now = np.empty((len(t), S)), np.zeros(len(t), dtype=bool), t0
    for tau in sorted({e[0] for e in events if e[0] > t0}) + [None]:
        end = t[-1] if tau is None else tau
        take = ~done & (t <= end)
        ys = R.radau(S, reactions, k, y, np.r_[t[take], end], t0=now, **kw)
        out[take], done = ys[:-1], done | take
        y, now = ys[-1].copy(), end
        if tau is not None:
            intervene(y, tau)
    assert done.all()
    return out


def radau_observed(args):
    """(S, reactions, y0, t, events, t0, observables, x) -> the observables [T, O] at the log10 constants x; one argument, for a process pool"""
    S, rx, y0, t, events, t0, obs, x = args
    return piecewise_radau(S, rx, R.rate_constants(rx, x, "log10"), y0, t, events, t0) @ np.asarray(obs, dtype=float).T


def _network(name):
    """(S, reactions, y0, t, observables, nominal, sd_rel, lanes) of a named network"""
    if name == "mm":
        return 4, NW.MM_REACTIONS, NW.MM_Y0, NW.MM_T, CN.MM_OBSERVABLES, NW.MM_NOMINAL, 0.05, 1
    if name == "chain8":
        return 8, NW.CHAIN_REACTIONS, NW.CHAIN_Y0, NW.CHAIN_T, np.eye(8), NW.CHAIN_NOMINAL, 0.02, 1
    if name == "enzyme13":
        return 13, W.ENZ.REACTIONS, W.ENZ.Y0, W.ENZ.TSPAN, W.ENZ.OBSERVABLES, W.ENZ.NOMINAL, 0.03, 16
    rx, y0, obs = W.chain_network(17)
    return 17, rx, y0, W.CHAIN_T, obs, W.CHAIN_NOMINAL, 0.03, 32


EVENTS = dict(mm=MM_EVENTS, chain8=CHAIN8_EVENTS, enzyme13=ENZ_EVENTS, chain17=CHAIN17_EVENTS)


@functools.lru_cache(maxsize=None)
def _data(name, y0, events, t0):
    """The observables [O, T] of a named network from the start y0 under the events, at the nominal constants (cached: tests share them)"""
    S, rx, _, t, obs, nominal, _, _ = _network(name)
    return radau_observed((S, rx, np.array(y0), t, events, t0, obs, nominal)).T.copy()


def single(name, events="own", y0=None, t0=0.0, **kw):
    """The named network as a single experiment with the events (default: the network's own above) given to the constructor; the data are
    piecewise Radau's under these events.  events=None: the keyword is not passed at all."""
    S, rx, own_y0, t, obs, _, sd_rel, lanes = _network(name)
    y0 = np.asarray(own_y0 if y0 is None else y0, dtype=float)
    events = EVENTS[name] if isinstance(events, str) else events
    data = _data(name, tuple(y0), tuple(events or ()), float(t0))
    kw.setdefault("lanes_per_point", lanes)
    if events is not None:
        kw["events"] = list(events)
    return MassActionODELogLike(S, rx, y0, t, obs, data, sd_rel * np.abs(data) + 0.01, t0=t0, **kw)


def conditions(name, values, events, **kw):
    """(multi, one): `name` under one condition per entry of `values` (MM: the substrate's dose; enzyme13: the scale of substrate A), the
    condition c with events[c]; one(c, **kw2) is the single-experiment object of condition c with the same data."""
    S, rx, y0, t, obs, _, sd_rel, lanes = _network(name)
    conds = []
    for v, ev in zip(values, events):
        y = np.array(y0, dtype=float)
        if name == "mm":
            y[1] = v
        else:
            y[W.ENZ.A] *= v
        data = _data(name, tuple(y), tuple(ev), 0.0)
        conds.append(dict(y0=y, data=data, sd=sd_rel * np.abs(data) + 0.01, events=list(ev)))
    multi = MassActionODELogLike(S, rx, None, t, obs, None, None, lanes_per_point=lanes, conditions=conds, **kw)

    def one(c, **kw2):
        cond = conds[c]
        return MassActionODELogLike(S, rx, cond["y0"], t, obs, cond["data"], cond["sd"], lanes_per_point=lanes, events=cond["events"], **dict(kw, **kw2))
    return multi, one


def mm_conditions(**kw):
    return conditions("mm", CN.MM_DOSES, MM_CONDITION_EVENTS, **kw)


def enzyme13_conditions(**kw):
    return conditions("enzyme13", (0.5, 1.0, 2.0), ENZ_CONDITION_EVENTS, **kw)
