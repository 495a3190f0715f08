"""Networks for the tests of MassActionODELogLike(equilibrate=...): the networks of ode_networks, ode_wide_networks, ode_wave_networks
and ode_event_networks equilibrated to their resting state before the experiment, alone and under three conditions (phase off / on / on
with a bolus at t0), and a Brusselator as a mass-action network (a steady state below the Hopf point, a limit cycle above it).  All
synthetic: the data are the host build's own tight simulation at the nominal constants -- they only define a likelihood; what the tests
compare against is numpy's restatement of the steady-state test, scipy's Radau and the host build's bits."""
import functools

import numpy as np

from pydream_amd.likelihoods import MassActionODELogLike

from . import ode_event_networks as EV
from . import ode_wave_networks as WV
from . import ode_wide_networks as W

# the stimulus of a condition: a bolus at t0 = 0 (substrate for MM and enzyme13, the first species of a chain)
BOLUS = dict(mm=(0.0, 1, 1.0, 2.0), chain8=(0.0, 0, 1.0, 1.0), enzyme13=(0.0, W.ENZ.A, 1.0, 2.0), chain17=(0.0, 0, 1.0, 1.0))
# A budget of the phase's attempted steps at which, in the +-1 decade box around MM's nominal constants, some points are not steady
# yet and others are (chosen on the host build: test_ode_equilibrate_cpu.test_a_starved_phase_fails_some_points_and_not_others)
MM_STARVED_EQUILIBRATE_STEPS = 240

# X -> A, A -> B (rate B), 2A + B -> 3A, A -> X with linear rate constants k = (1, B, 1, 1): the steady state (1, B), stable for B < 2
BRUSSELATOR_REACTIONS = [({}, {0: 1}, 0), ({0: 1}, {1: 1}, 1), ({0: 2, 1: 1}, {0: 3}, 2), ({0: 1}, {}, 3)]
BRUSSELATOR_T = np.linspace(0.0, 10.0, 11)


def network(name):
    """(S, reactions, y0, t, observables, nominal, sd_rel, lanes) of a named network: ode_event_networks' four, and "chainS" at 64 lanes"""
    if name in EV.EVENTS:
        return EV._network(name)
    S = int(name[5:])
    rx, y0, obs = W.chain_network(S)
    return S, rx, y0, W.CHAIN_T, obs, W.CHAIN_NOMINAL, 0.03, WV.LANES


def smallest_wave_chain():
    """the name of the smallest chain among ode_wave_networks.CASES"""
    return "chain%d" % min(case[3][0] for name, case in WV.CASES.items() if name.startswith("chain"))


def _frozen(eq):
    return tuple(sorted(eq.items())) if hasattr(eq, "items") else eq


@functools.lru_cache(maxsize=None)
def _data(name, y0, events, eq, t0):
    """The observables [O, T] of the named network at the nominal constants from y0 under the events, equilibrated first if eq says so:
    the host build at tight tolerances (cached: the tests share them)."""
    S, rx, _, t, obs, nominal, _, lanes = network(name)
    eq = dict(eq) if isinstance(eq, tuple) else eq
    if eq:                                  # (the data's own phase: tight, whatever budget the object under test is given)
        eq = dict(horizon=(eq if isinstance(eq, dict) else {}).get("horizon", max(float(t[-1]) - t0, 1e-300)), max_steps=20000)
    tight = MassActionODELogLike(S, rx, np.array(y0), t, obs, np.zeros((len(obs), len(t))), 1.0, t0=t0, lanes_per_point=lanes, events=list(events),
                                 equilibrate=eq or None, rtol=1e-10, atol=1e-12, max_steps=20000)
    sim = tight.simulate(nominal)[0]
    assert np.all(np.isfinite(sim)), name
    return sim.T.copy()


def experiment(name, equilibrate=True, events=(), y0=None, t0=0.0):
    """dict(y0, data, sd, events, equilibrate) of one experiment of the named network"""
    _, _, own_y0, _, _, _, sd_rel, _ = network(name)
    y0 = np.asarray(own_y0 if y0 is None else y0, dtype=float)
    data = _data(name, tuple(y0), tuple(events), _frozen(equilibrate), float(t0))
    return dict(y0=y0, data=data, sd=sd_rel * np.abs(data) + 0.01, events=list(events), equilibrate=equilibrate)


def single(name, equilibrate=True, events=(), y0=None, t0=0.0, **kw):
    """The named network as one experiment that equilibrates first (equilibrate: what the constructor gets)."""
    S, rx, _, t, obs, _, _, lanes = network(name)
    e = experiment(name, equilibrate, events, y0, t0)
    return MassActionODELogLike(S, rx, e["y0"], t, obs, e["data"], e["sd"], t0=t0, lanes_per_point=lanes, events=e["events"],
                                equilibrate=equilibrate, **kw)


def plain_from(like, y0, **kw):
    """The experiment of `like` without the phase, started from y0: the same network, times, data and events.  y0 goes straight into
    the object's block (the source does not hold it): a resting state may carry an amount that is negative within the solver's
    tolerance, -(atol + rtol |y|) at most, which the constructor would refuse as a start amount."""
    plain = MassActionODELogLike(like.n_species, like.reactions, like.y0, like.t, like.observables, like.data, like.sd, rate_scale=like.rate_scale,
                                 t0=like.t0, rtol=like.rtol, atol=like.atol, max_steps=like.max_steps, lanes_per_point=like.lanes_per_point,
                                 events=like.events, **kw)
    plain.y0 = np.array(y0, dtype=float)
    return plain


def conditions(name, equilibrate=True, t0=0.0, **kw):
    """(multi, one): the named network under three conditions -- the phase off, on, and on with the network's BOLUS at t0 --; one(c) is
    the single-experiment object of condition c.  equilibrate: the setting of the two conditions that have the phase."""
    S, rx, _, t, obs, _, _, lanes = network(name)
    bolus = (float(t0),) + BOLUS[name][1:]
    exps = [experiment(name, False, (), None, t0), experiment(name, equilibrate, (), None, t0), experiment(name, equilibrate, (bolus,), None, t0)]
    multi = MassActionODELogLike(S, rx, None, t, obs, None, None, t0=t0, lanes_per_point=lanes, conditions=exps, **kw)

    def one(c, **kw2):
        e = exps[c]
        return MassActionODELogLike(S, rx, e["y0"], t, obs, e["data"], e["sd"], t0=t0, lanes_per_point=lanes, events=e["events"],
                                    equilibrate=e["equilibrate"], **dict(kw, **kw2))
    return multi, one


def brusselator(y0, horizon=10.0, **eq):
    """The Brusselator from y0, equilibrated with the given horizon (and further settings of the phase); data 1, sd 1."""
    return MassActionODELogLike(2, BRUSSELATOR_REACTIONS, y0, BRUSSELATOR_T, np.eye(2), np.ones((2, len(BRUSSELATOR_T))), 1.0, rate_scale="linear",
                                equilibrate=dict(horizon=horizon, **eq))
