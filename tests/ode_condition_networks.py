"""Networks measured under several experimental conditions, for the tests of MassActionODELogLike(conditions=...): each builder
returns (the multi-condition object, a function c -> the single-condition object of condition c made the way the class has always been
made).  All synthetic: the data of every condition come from scipy's Radau at the nominal constants from that condition's start."""
import functools

import numpy as np

from pydream_amd.likelihoods import MassActionODELogLike

from . import ode_networks as NW
from . import ode_wide_networks as W

MM_OBSERVABLES = [[0, 1, 0, 0], [0, 0, 0, 1]]
MM_DOSES = (0.5, 2.0, 8.0)
MM_DOSES_5 = (0.5, 2.0, 8.0, 0.0, 32.0)             # (a condition without substrate: nothing happens, the data are y0's observables)


@functools.lru_cache(maxsize=None)
def _radau_observed(name, scale_or_dose):
    """The observables [O, T] at the nominal constants for one condition of a named network (cached: several tests share them)."""
    S, rx, y0, t, obs, nominal = _network(name, scale_or_dose)
    return (NW.radau(S, rx, y0, t, nominal) @ np.asarray(obs, dtype=float).T).T.copy()


def _network(name, v):
    if name == "mm":
        return 4, NW.MM_REACTIONS, [0.5, v, 0.0, 0.0], NW.MM_T, MM_OBSERVABLES, NW.MM_NOMINAL
    if name == "chain8":
        return 8, NW.CHAIN_REACTIONS, v * np.asarray(NW.CHAIN_Y0), NW.CHAIN_T, np.eye(8), NW.CHAIN_NOMINAL
    if name == "enzyme13":                           # the substrate A scaled
        y0 = W.ENZ.Y0.copy()
        y0[W.ENZ.A] *= v
        return 13, W.ENZ.REACTIONS, y0, W.ENZ.TSPAN, W.ENZ.OBSERVABLES, W.ENZ.NOMINAL
    S = int(name[5:])                                # "chain17", "chain32": ode_wide_networks' chain, every start amount scaled
    rx, y0, obs = W.chain_network(S)
    return S, rx, v * y0, W.CHAIN_T, obs, W.CHAIN_NOMINAL


def build(name, values, sd_rel, lanes=1, unobserved=(), **kw):
    """(multi, single): `name` under one condition per entry of `values` (a dose or a scale of the start amounts), sd = sd_rel |data| +
    0.01; unobserved: (condition, observable, time) entries set to NaN.  The multi-condition object gets everything through its
    conditions (the constructor's y0, data and sd are None); single(c, **kw2) is condition c alone."""
    conds, shared = [], None
    for c, v in enumerate(values):
        S, rx, y0, t, obs, _ = _network(name, v)
        data = _radau_observed(name, v).copy()
        for cc, o, j in unobserved:
            if cc == c:
                data[o, j] = np.nan
        conds.append(dict(y0=np.asarray(y0, dtype=float), data=data, sd=sd_rel * np.abs(data) + 0.01))
        shared = (S, rx, t, obs)
    S, rx, t, obs = shared
    multi = MassActionODELogLike(S, rx, None, t, obs, None, None, lanes_per_point=lanes, conditions=conds, **kw)

    def single(c, **kw2):
        return MassActionODELogLike(S, rx, conds[c]["y0"], t, obs, conds[c]["data"], conds[c]["sd"], lanes_per_point=lanes, **dict(kw, **kw2))
    return multi, single


def mm(doses=MM_DOSES, **kw):
    return build("mm", tuple(doses), 0.05, unobserved=((1, 0, 3),), **kw)


def enzyme13(scales=(0.5, 1.0, 2.0), **kw):
    return build("enzyme13", tuple(scales), 0.03, lanes=16, **kw)


def chain(S, lanes, scales, **kw):
    return build("chain%d" % S, tuple(scales), 0.02 if S == 8 else 0.03, lanes=lanes, **kw)


def left_to_right(columns):
    """((l_0 + l_1) + l_2) + ... of the columns of an [n, C] array"""
    total = columns[:, 0].copy()
    for c in range(1, columns.shape[1]):
        total = total + columns[:, c]
    return total
