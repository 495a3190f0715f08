"""Networks whose conditions carry "params", a view of the point per condition, for the tests of MassActionODELogLike's
condition-specific parameters (a plain module: nothing here is collected).  Built on ode_condition_networks (mm, enzyme13, the chains),
ode_wave_networks (the smallest wave chain) and ode_combined_networks (every kind of reader in one object).  Every builder returns
(multi, single, mappings): the object with views, c -> the object of condition c alone made WITHOUT "params" -- what the contract
compares item c with, at the row V_c x --, and the declared mappings, from which the tests compute V_c X themselves (viewed()).

The basic networks have n0 sampled constants.  One reaction's rate becomes Monomial({i: 1, F: 1}) with F = n0 + 1 a FORMAL index, fixed
in every condition (0.0: the bare rate's bits; -0.5: a known knock-down); the point gets one more coordinate, n0, which one condition
reads in the place of another rate (a mapping to another coordinate); and one condition fixes a rate at a number.  So d = n0 + 1 and
P = n0 + 2 > d."""
import functools

import numpy as np

from pydream_amd.likelihoods import MassActionODELogLike, Monomial

from . import ode_combined_networks as CB
from . import ode_condition_networks as CN
from . import ode_equilibrate_networks as EQ
from . import ode_networks as NW
from . import ode_wide_networks as W

WAVE = EQ.smallest_wave_chain()                      # "chain33"
STARVED_MAX_STEPS = 60                               # mm: some items of a point fail, others do not


def viewed(mappings, c, X, P):
    """V_c X by numpy indexing from the declared mapping: [n, P]; an index without an entry is itself (0 where the point has no such
    coordinate: nothing reads it)."""
    X = np.asarray(X, dtype=float)
    out = np.zeros((len(X), P))
    for i in range(P):
        target = mappings[c].get(i, i)
        if isinstance(target, float):
            out[:, i] = target
        elif target < X.shape[1]:
            out[:, i] = X[:, target]
    return out


def _spec(name):
    """(lanes, the values of the conditions, sd_rel, nominal, the rate index whose first reaction gets the formal factor, the rate index
    read from the extra coordinate, the rate index fixed at a number)"""
    if name == "mm":
        return 1, CN.MM_DOSES, 0.05, NW.MM_NOMINAL, 2, 0, 1
    if name == "enzyme13":
        return 16, (0.5, 1.0, 2.0), 0.03, W.ENZ.NOMINAL, 1, 0, 2
    if name == "chain17":
        return 32, (1.0, 2.0), 0.03, W.CHAIN_NOMINAL, 16, 3, 9
    assert name == WAVE
    return 64, (0.5, 1.0, 2.0), 0.03, W.CHAIN_NOMINAL, 16, 3, 9


def mappings_of(name, identity=False, values=None):
    lanes, own, _, nominal, r_formal, i_moved, i_fixed = _spec(name)
    values = own if values is None else values
    n0 = len(nominal)
    F = n0 + 1
    if identity:
        return [{i: i for i in range(n0)} for _ in values]
    maps = [{F: 0.0}, {F: -0.5, i_moved: n0}, {F: 0.0, i_fixed: float(nominal[i_fixed]) + 0.125}]
    if len(values) == 2:                             # (two conditions: the three kinds of target between them)
        maps = [{F: 0.0, i_moved: n0}, {F: -0.5, i_fixed: float(nominal[i_fixed]) + 0.125}]
    return maps


def nominal_of(name):
    """the nominal point of the object with views: the network's constants and the extra coordinate at the moved rate's own value"""
    _, _, _, nominal, _, i_moved, _ = _spec(name)
    return np.r_[nominal, nominal[i_moved]]


def points(name, n, seed, width=1.0, outside=0.0):
    return NW.box_points(nominal_of(name), n, seed, width=width, outside=outside)


def basic(name, view=True, identity=False, maps=None, values=None, **kw):
    """(multi, single, mappings) of a basic network.  view=False: the twin without "params" -- the same reactions, the formal factor's
    index a plain coordinate; identity: explicit {i: i} mappings on the network as it always was (no formal factor); maps: the
    conditions' mappings where they are not mappings_of(name); values: the conditions' doses or scales where they are not the
    network's own."""
    lanes, own, sd_rel, nominal, r_formal, _, _ = _spec(name)
    values = own if values is None else values
    n0 = len(nominal)
    net = name
    S, rx, _, t, obs, _ = CN._network(net, values[0])
    rx = list(rx)
    if not identity:
        j = next(r for r, reaction in enumerate(rx) if isinstance(reaction[2], (int, np.integer)) and reaction[2] == r_formal)
        rx[j] = (rx[j][0], rx[j][1], Monomial({rx[j][2]: 1, n0 + 1: 1}))
    maps = mappings_of(name, identity, values) if maps is None else maps
    conds = []
    for c, v in enumerate(values):
        data = CN._radau_observed(net, v).copy()
        cond = dict(y0=np.asarray(CN._network(net, v)[2], dtype=float), data=data, sd=sd_rel * np.abs(data) + 0.01)
        if view:
            cond["params"] = maps[c]
        conds.append(cond)
    multi = MassActionODELogLike(S, rx, None, t, obs, None, None, lanes_per_point=lanes, conditions=conds, **kw)

    def single(c, **kw2):
        return MassActionODELogLike(S, rx, conds[c]["y0"], t, obs, conds[c]["data"], conds[c]["sd"], lanes_per_point=lanes, **dict(kw, **kw2))
    return multi, single, maps


# ---- every kind of reader through the view: ode_combined_networks' small full case of each build, without its constraint
READER_EXTRA = (CB.P_K, CB.P_SCALE, 0, CB.P_SIGMA, CB.P_Y0)          # the coordinates 10..14 stand in for these indices
READER_D = CB.NDIM + len(READER_EXTRA)


def reader_mappings(case):
    nom = case.nominal
    return [{CB.P_K: 10, CB.P_SCALE: 11},                                   # (equilibrates) a Hill K, the Monomial scale
            {0: 12, CB.P_GAIN: float(nom[CB.P_GAIN]) + 0.0625, CB.P_SIGMA: 13},     # the Monomial rate, the gains, a Noise sigma
            {CB.P_Y0: 14, CB.P_REL: float(nom[CB.P_REL]), 1: 1}]               # (equilibrates) the y0 Monomial, a Noise rel, an identity


@functools.lru_cache(maxsize=None)
def readers(lanes, view=True):
    """(multi, single, mappings, case): a Monomial rate, a y0 Monomial, a Monomial scale, Noise sigma and rel, Hill Ks and input gains,
    each remapped in some condition; conditions 0 and 2 equilibrate.  view=False: the twin without "params"."""
    case = CB.starved_case(lanes)
    data, maps = case.data(), reader_mappings(case)
    shared = dict(rate_scale=case.rate_scale, t0=case.t0, lanes_per_point=lanes, scale=case.scale, noise=case.noise)
    conds = [dict(data=data[0][0], sd=data[0][1], events=[]),
             dict(data=data[1][0], sd=data[1][1], y0=case.y0[1], equilibrate=False, inputs=case.inputs[1]),
             dict(data=data[2][0], sd=data[2][1], events=case.events[2], equilibrate=CB.EQUILIBRATE[2], inputs=case.inputs[2])]
    for c, cond in enumerate(conds):
        if view:
            cond["params"] = maps[c]
    multi = MassActionODELogLike(case.S, case.reactions, case.y0[0], case.t, case.observables, None, None, conditions=conds,
                                 inputs=case.inputs[0], events=case.own_events, equilibrate=True, **shared)

    def single(c):
        d, sd = data[c]
        return MassActionODELogLike(case.S, case.reactions, case.y0[c], case.t, case.observables, d, sd, inputs=case.inputs[c],
                                    events=case.events[c], equilibrate=(True, False, CB.EQUILIBRATE[2])[c], **shared)
    return multi, single, maps, case


def reader_points(lanes, n, seed, width=0.5):
    case = CB.starved_case(lanes)
    nominal = np.r_[case.nominal, case.nominal[list(READER_EXTRA)]]
    return NW.box_points(nominal, n, case.seed * 7 + seed, width=width)


# ---- mm on three gels: a sampled readout scale per gel and a known knock-down of kcat in the second condition
GEL_SCALES = np.log10([1.0, 1.5, 0.7])
GEL_NOMINAL = np.r_[NW.MM_NOMINAL, GEL_SCALES]       # d = 6: the three rate constants and a scale per gel; the formal index 6 is the knock-down


def mm_gels(**kw):
    """(multi, mappings): scale=[Monomial({3: 1}), 1.0] with 3 -> 3 + gel, and kcat as Monomial({2: 1, 6: 1}) with the formal index 6
    fixed at 0.0, -0.5, 0.0"""
    rx = list(NW.MM_REACTIONS)
    rx[2] = (rx[2][0], rx[2][1], Monomial({2: 1, 6: 1}))
    maps = [{3: 3 + c, 6: (0.0, -0.5, 0.0)[c]} for c in range(3)]
    conds = []
    for c, dose in enumerate(CN.MM_DOSES):
        data = CN._radau_observed("mm", dose).copy()
        data[0] *= 10.0 ** GEL_SCALES[c]
        conds.append(dict(y0=[0.5, dose, 0.0, 0.0], data=data, sd=0.05 * np.abs(data) + 0.01, params=maps[c]))
    return MassActionODELogLike(4, rx, None, NW.MM_T, CN.MM_OBSERVABLES, None, None, conditions=conds, scale=[Monomial({3: 1}), 1.0], **kw), maps
