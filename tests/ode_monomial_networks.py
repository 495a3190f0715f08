"""Networks whose rate constants, start amounts, observable scales and constraints are likelihoods.Monomial products of the sampled
constants, for the tests of that construct.  A SPEC says everything an independent reference needs (reference_loglike below reads the
spec alone, never the generated code); build(spec) returns (the object, single(c, constraints=...) -> the single-condition object of
condition c).  All synthetic: the data of every condition come from scipy's Radau at the nominal point, sd = rel |data| + 0.01.

A spec with the key "events" (a list of (time, species, factor, amount) per condition: the *_events specs) combines Monomials with dosing
and wash-out events; its data and its reference come from Radau restarted at every event (ode_event_networks.piecewise_radau)."""
import functools

import numpy as np

from pydream_amd.likelihoods import MassActionODELogLike, Monomial

from . import ode_networks as NW
from . import ode_reference as REF
from . import ode_wide_networks as W


def mono_value(m, x):
    """10.0**(c + sum e x) in numpy, from the value object's own fields"""
    return 10.0 ** (m.log10_factor + sum(e * x[i] for i, e in m.exponents))


def constants(reactions, x):
    return np.array([mono_value(r, x) if isinstance(r, Monomial) else 10.0 ** x[r] if isinstance(r, (int, np.integer)) else r
                     for _, _, r in reactions], dtype=float)


def numbers(entries, x):
    """a y0 or a scale as doubles at the point x"""
    return np.array([mono_value(v, x) if isinstance(v, Monomial) else v for v in entries], dtype=float)


def events_of(spec, c):
    """condition c's events (time, species, factor, amount) in a spec that has them (the key "events": a list per condition), else none"""
    return tuple(spec["events"][c]) if spec.get("events") else ()


def radau_observed(spec, c, x, rtol=1e-12, atol=1e-14):
    """what is compared with condition c's data at the point x, [O, T]: scale * observables of a scipy Radau solution -- restarted at
    every event of the condition (ode_event_networks.piecewise_radau: the state changed by hand in between) where the spec has events"""
    k, y0 = constants(spec["reactions"], x), numbers(spec["y0"][c], x)
    if events_of(spec, c):
        from .ode_event_networks import piecewise_radau
        y = piecewise_radau(spec["S"], spec["reactions"], k, y0, spec["t"], events_of(spec, c), rtol=rtol, atol=atol)
    else:
        y = REF.radau(spec["S"], spec["reactions"], k, y0, spec["t"], rtol=rtol, atol=atol)
    scale = np.ones(len(spec["obs"])) if spec["scale"] is None else numbers(spec["scale"], x)
    return (y @ np.asarray(spec["obs"], dtype=float).T).T * scale[:, None]


def reference_loglike(spec, data, sd, x):
    """(the log-likelihood of x, the sum of its terms' magnitudes) from scipy alone: Radau at rtol 1e-10 (restarted at every event of a
    condition, where the spec gives per-condition events) and norm.logpdf for the data of every condition and for the constraints"""
    from scipy.stats import norm
    total = magnitude = 0.0
    for c in range(len(spec["y0"])):
        seen = np.isfinite(data[c])
        terms = norm(loc=data[c][seen], scale=sd[c][seen]).logpdf(radau_observed(spec, c, x, rtol=1e-10)[seen])
        total, magnitude = total + float(np.sum(terms)), magnitude + float(np.sum(np.abs(terms)))
    for m, loc, s in spec["constraints"]:
        term = float(norm(loc, s).logpdf(mono_value(m, x)))
        total, magnitude = total + term, magnitude + abs(term)
    return total, magnitude


def _mm_kd(knock_out=True):
    """E + S <-> ES -> E + P with x = [log kf, log KD, log kcat, log E0, log scale]: kr = KD kf, the enzyme's amount and the product's
    scale sampled, kcat / KD constrained; the doses 0.5, 2 and 8, the last one without enzyme (a plain 0.0 over the monomial).  Nothing
    happens without enzyme, so that condition's integration cannot run out of steps; knock_out=False ("mm_kd_doses") keeps the enzyme
    in all three, for the tests that need points failing in every condition."""
    rx = [({0: 1, 1: 1}, {2: 1}, 0), ({2: 1}, {0: 1, 1: 1}, Monomial({0: 1, 1: 1})), ({2: 1}, {0: 1, 3: 1}, 2)]
    e0 = Monomial({3: 1})
    return dict(S=4, reactions=rx, y0=[[e0, 0.5, 0.0, 0.0], [e0, 2.0, 0.0, 0.0], [0.0 if knock_out else e0, 8.0, 0.0, 0.0]], t=NW.MM_T,
                obs=[[0, 1, 0, 0], [0, 0, 0, 1]], scale=[1.0, Monomial({4: 1})], constraints=[(Monomial({2: 1, 1: -1}), 7.2, 1.5)],
                nominal=np.log10([3.0, 0.5 / 3.0, 1.2, 0.5, 2.0]), rel=0.05, lanes=1, unobserved=((1, 0, 3),))


def _enzyme13_m():
    """examples/enzyme's network, four backward rates as two-index monomials with a factor (one exponent 0.5), the enzyme's amount (x[20])
    and P's scale (x[21]) sampled, the two first-site turnover constants' ratio constrained; the other start amounts at 0.5, 1 and 2 times"""
    rx = list(W.ENZ.REACTIONS)
    for j, m in ((1, Monomial({0: 1, 1: 1}, -2.0)), (4, Monomial({3: 1, 4: 1}, -2.0)), (7, Monomial({6: 0.5, 7: 1}, -0.5)),
                 (19, Monomial({18: 1, 19: 1}, -np.log10(50.0)))):
        rx[j] = (rx[j][0], rx[j][1], m)
    y0 = []
    for v in (0.5, 1.0, 2.0):
        row = [float(a) for a in v * W.ENZ.Y0]
        row[W.ENZ.E] = Monomial({20: 1})
        y0.append(row)
    return dict(S=13, reactions=rx, y0=y0, t=W.ENZ.TSPAN, obs=W.ENZ.OBSERVABLES, scale=[Monomial({21: 1}), 1.0, 1.0, 1.0],
                constraints=[(Monomial({2: 1, 5: -1}), 1.3 / 1.2, 0.2)], nominal=np.r_[W.ENZ.NOMINAL, np.log10([0.05, 1.5])], rel=0.03, lanes=16,
                unobserved=())


def _chain17_m():
    """ode_wide_networks' chain of 17 species, one backward rate and the second cross link as monomials with a factor, species 0's
    amount (x[18]) and the fourth observable's scale (x[19]) sampled, one constraint; every other start amount at 1 and 2 times"""
    rx, y0, obs = W.chain_network(17)
    rx[16] = (rx[16][0], rx[16][1], Monomial({0: 1, 8: 1}, -np.log10(0.5)))
    rx[33] = (rx[33][0], rx[33][1], Monomial({16: 1, 17: 1}, -np.log10(3.0)))
    starts = []
    for v in (1.0, 2.0):
        row = [float(a) for a in v * y0]
        row[0] = Monomial({18: 1})
        starts.append(row)
    scale = [1.0] * len(obs)
    scale[3] = Monomial({19: 1})
    return dict(S=17, reactions=rx, y0=starts, t=W.CHAIN_T, obs=obs, scale=scale, constraints=[(Monomial({1: 1, 9: -1}), 0.7 / 0.15, 0.5)],
                nominal=np.r_[W.CHAIN_NOMINAL, np.log10([1.0, 0.7])], rel=0.03, lanes=32, unobserved=())


def _dense8_m():
    """ode_wide_networks.dense_network's recipe at 8 species and 24 reactions (the one-lane long form), every fourth rate a monomial of
    two parameters; a single experiment (data 1, sd 1 at three times) with one start amount sampled and one constraint"""
    rng = np.random.default_rng(1)
    rx = []
    for j in range(24):
        a, b, c = (int(s) for s in rng.choice(8, 3, replace=False))
        rate = Monomial({j % 20: 1, (j + 7) % 20: -0.5}, 0.125) if j % 4 == 1 else j % 20
        rx.append(({a: 1, b: 1}, {c: 1}, rate) if j % 2 == 0 else ({c: 1}, {a: 1, b: 1}, rate))
    y0 = [float(a) for a in np.linspace(0.2, 1.0, 8)]
    y0[2] = Monomial({3: 1, 4: -1}, np.log10(0.4))
    return dict(S=8, reactions=rx, y0=[y0], t=np.array([0.1, 0.4, 1.0]), obs=np.eye(8)[:4], scale=None,
                constraints=[(Monomial({0: 1, 1: 1}), 1.0, 0.5)], nominal=np.zeros(20), rel=None, lanes=1, unobserved=(), single=True)


def _mm_kd_events():
    """mm_kd with a different event list in each of its three conditions: condition 0 changes the ENZYME -- the species whose start is a
    Monomial -- at t0 (half of it plus 0.1) and gets a bolus of substrate strictly between the outputs 6.0 and 6.5; condition 1 gets one
    exactly on the output time 2.0, whose substrate reading is the one left unobserved (NaN); condition 2 (the knock-out) has none, so
    its block is padded to two events"""
    spec = _mm_kd()
    return dict(spec, events=[[(0.0, 0, 0.5, 0.1), (6.2, 1, 1.0, 1.0)], [(float(spec["t"][3]), 1, 1.0, 1.5)], []])


def _enzyme13_m_events():
    """enzyme13_m (16 lanes) with ode_event_networks' 0, 1 and 3 events in its three conditions"""
    from .ode_event_networks import ENZ_CONDITION_EVENTS
    return dict(_enzyme13_m(), events=[list(ev) for ev in ENZ_CONDITION_EVENTS])


def _chain17_m_events():
    """chain17_m (32 lanes): no events in its first condition, ode_event_networks' wash-out and set-to-value in the second"""
    from .ode_event_networks import CHAIN17_EVENTS
    return dict(_chain17_m(), events=[[], list(CHAIN17_EVENTS)])


SPECS = {"mm_kd": _mm_kd, "mm_kd_doses": lambda: _mm_kd(False), "enzyme13_m": _enzyme13_m, "chain17_m": _chain17_m, "dense8_m": _dense8_m,
         "mm_kd_events": _mm_kd_events,
         "enzyme13_m_events": _enzyme13_m_events,
         "chain17_m_events": _chain17_m_events}


@functools.lru_cache(maxsize=None)
def spec_and_data(name):
    """(spec, data [C, O, T], sd [C, O, T]) of a named network: computed once, shared by the tests, not to be written to"""
    spec = SPECS[name]()
    C, O, T = len(spec["y0"]), len(spec["obs"]), len(spec["t"])
    if spec["rel"] is None:
        data, sd = np.ones((C, O, T)), np.ones((C, O, T))
    else:
        data = np.stack([radau_observed(spec, c, spec["nominal"]) for c in range(C)])
        for c, o, j in spec["unobserved"]:
            data[c, o, j] = np.nan
        sd = spec["rel"] * np.abs(data) + 0.01
    for a in (data, sd):
        a.setflags(write=False)
    return spec, data, sd


def build(name, **kw):
    """(the object of the named network, single): single(c, constraints=True, **kw2) is condition c alone as a single experiment, with
    or without the constraints."""
    spec, data, sd = spec_and_data(name)
    shared = dict(dict(lanes_per_point=spec["lanes"], scale=spec["scale"]), **kw)

    def single(c, constraints=True, **kw2):
        ev = dict(events=list(events_of(spec, c))) if spec.get("events") else {}
        return MassActionODELogLike(spec["S"], spec["reactions"], spec["y0"][c], spec["t"], spec["obs"], data[c], sd[c],
                                    constraints=spec["constraints"] if constraints else None, **dict(shared, **ev, **kw2))
    if spec.get("single"):
        return single(0), single
    conds = [dict(y0=spec["y0"][c], data=data[c], sd=sd[c], **(dict(events=list(events_of(spec, c))) if spec.get("events") else {})) for c in range(len(spec["y0"]))]
    return MassActionODELogLike(spec["S"], spec["reactions"], None, spec["t"], spec["obs"], None, None, conditions=conds,
                                constraints=spec["constraints"], **shared), single


def nominal(name):
    return spec_and_data(name)[0]["nominal"]
